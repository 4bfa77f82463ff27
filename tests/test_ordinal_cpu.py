"""CPU checks of the ordinal (cumulative-logit) regression target (NF_TARGET_ORDINAL_LOGIT, kind 32): the constant (header, Python
mirror, Julia extension) with the ABI, the symbol list and the target descriptor unchanged, nf_target_check's conventions as
nf_target_logp reports them BEFORE any device work (a stand-in context is enough), the refusals of the flows that evaluate their
target in their own kernels, the host packing (sorted, block-uniform labels, padding of weight exactly 0, n_k, an empty category, a
row count that is no multiple of 32), the constructor's refusals, unpack / predict, the routing of the Python mirror, the numpy form
against central differences, against the unfactored definition and -- at C = 2 -- against logistic regression, the float32 floor
of the GPU tests' inputs, and the new kernels' resources."""
import ctypes as C
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

import glm_forms as gf
import ordinal_forms as of
import parity as P
from __graft_entry__ import ROOT, build, load_package

KIND = 32


@pytest.fixture(scope="module")
def nf():
    build()  # no-op when libnfhip.so is up to date
    return load_package()


def _standin():
    return C.cast((C.c_char * 4096)(), C.c_void_p)


def _t(a, dtype=torch.float64):
    return torch.tensor(np.asarray(a), dtype=dtype)


def make_target(nf, X, lab, off, wt, Cn, dtype=torch.float64, **kw):
    kw = {"prior_sigma": of.SIGMA_BETA, "cut_sigma": of.SIGMA_CUT, "cut_loc": of.CUT_LOC, **kw}
    return nf.OrdinalRegressionTarget(_t(X, dtype), torch.tensor(np.asarray(lab)), Cn, offset=_t(off, dtype), weights=_t(wt, dtype), **kw)


def test_the_constant_matches_the_header_the_mirror_and_the_julia_extension(nf):
    hdr = open(os.path.join(ROOT, "include", "nfhip.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"^#define (NF_TARGET_\w+) (\d+)", hdr, re.M)}
    jl = open(os.path.join(ROOT, "ext", "NormalizingFlowsNFHipExt.jl")).read()
    m = re.search(r"const NF_TARGET_ORDINAL_LOGIT = Int32\((\d+)\)", jl)
    assert m and int(m.group(1)) == KIND
    # the header writes the kind relative to the one before it: #define NF_TARGET_ORDINAL_LOGIT (NF_TARGET_DGLM_NEGBIN + 1)
    e = re.search(r"^#define NF_TARGET_ORDINAL_LOGIT \((NF_TARGET_\w+) \+ (\d+)\)\s*$", hdr, re.M)
    assert e, "the header does not define NF_TARGET_ORDINAL_LOGIT"
    defs["NF_TARGET_ORDINAL_LOGIT"] = defs[e.group(1)] + int(e.group(2))
    assert defs["NF_TARGET_ORDINAL_LOGIT"] == nf._lib.NF_TARGET_ORDINAL_LOGIT == KIND == max(defs.values())
    assert len(set(defs.values())) == len(defs)  # no two kinds share a value
    for name, v in defs.items():
        assert getattr(nf._lib, name) == v
    assert nf.load_library().nf_abi_version() == 4
    assert len(nf.SYMBOLS) == 49
    assert [f[0] for f in nf._lib.Target._fields_] == ["kind", "p0", "p1", "s0", "s1"]


def test_target_check_errors_come_before_device_work(nf):
    """NF_ERR_ARG (-1) and NF_ERR_UNSUPPORTED (-2) for every violated convention without touching the context (N = 0: nothing is
    launched, and a good target's answer is no error)"""
    from normalizingflows_jl_amd._lib import Target

    lib = nf.load_library()
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p).value
    ctx = _standin()

    def logp(t, d=8, n=4, dtype=0):
        return lib.nf_target_logp(ctx, dtype, C.byref(t), d, n, C.c_void_p(p), C.c_void_p(p), None)

    for dtype in (0, 1):
        assert logp(Target(KIND, 0, p, 64.0, 5.0), dtype=dtype) == -1               # p0 = NULL
        assert logp(Target(KIND, p, 0, 64.0, 5.0), dtype=dtype) == -1               # p1 = NULL
        for s0 in (0.0, -32.0, 8.0, 33.0, 48.0, 32.5, 2147483648.0, 4294967296.0, math.nan, math.inf):
            assert logp(Target(KIND, p, p, s0, 5.0), dtype=dtype) == -1, s0         # not a positive multiple of 32 that fits an int
        for s1 in (0.0, 1.0, -3.0, 17.0, 2.5, math.nan, math.inf):
            assert logp(Target(KIND, p, p, 64.0, s1), d=40, dtype=dtype) == -1, s1  # not an integer in 2..16
        assert logp(Target(KIND, p, p, 64.0, 5.0), d=4, dtype=dtype) == -1          # d < C: no coefficient left
        assert logp(Target(KIND, p, p, 64.0, 2.0), d=1, dtype=dtype) == -1
        assert logp(Target(KIND, p, p, 33.0, 5.0), d=257, dtype=dtype) == -1        # an argument error first
        assert logp(Target(KIND, p, p, 64.0, 5.0), d=257, dtype=dtype) == -2        # d > 256
        assert logp(Target(KIND, p, p, 64.0, 16.0), d=300, n=0, dtype=dtype) == -2
        assert logp(Target(KIND, p, p, 64.0, 5.0), n=0, dtype=dtype) >= 0           # past the check
        assert logp(Target(KIND, p, p, 32.0, 2.0), d=2, n=0, dtype=dtype) >= 0      # the smallest: one coefficient, one cutpoint
        assert logp(Target(KIND, p, p, 32.0, 5.0), d=5, n=0, dtype=dtype) >= 0      # d = C
        assert logp(Target(KIND, p, p, 64.0, 16.0), d=256, n=0, dtype=dtype) >= 0   # C and d at their caps
        assert logp(Target(KIND, p, p, 2147483616.0, 2.0), n=0, dtype=dtype) >= 0   # the largest multiple of 32 below 2^31
    assert logp(Target(33, p, p, 64.0, 5.0)) == -1  # no such kind


def _five(lib, ctx, p, val, desc, tgt):
    return [lib.nf_elbo_value_and_grad(ctx, C.byref(desc), C.byref(tgt), p, p, 8, 8, 1, 0, 0, p),
            lib.nf_elbo_batch(ctx, C.byref(desc), C.byref(tgt), p, p, 8, None, C.byref(val)),
            lib.nf_elbo_batch_rng(ctx, C.byref(desc), C.byref(tgt), p, 8, 1, 0, 0, C.byref(val)),
            lib.nf_elbo_step(ctx, C.byref(desc), C.byref(tgt), p, p, p, 8, 1, 0, 1e-3, 0.9, 0.999, 1e-8, None, None),
            lib.nf_elbo_step_enqueue(ctx, C.byref(desc), C.byref(tgt), p, p, p, 8, 1, p, 1e-3, 0.9, 0.999, 1e-8, None)]


def test_flows_that_evaluate_the_target_in_their_own_kernels_refuse_before_device_work(nf):
    """planar, radial, mean-field and Hamiltonian descriptors answer NF_ERR_UNSUPPORTED (-2) at all five ELBO entry points, with the
    ordinal kind as the target and as the Hamiltonian score; a non-centring layer does not take it (NF_ERR_ARG) -- the stand-in
    context is never used."""
    from normalizingflows_jl_amd._lib import NF_KIND, FlowDesc, Target

    lib = nf.load_library()
    buf = (C.c_double * 256)()
    p = C.cast(buf, C.c_void_p)
    ctx = _standin()
    val = C.c_double(0.0)
    diag = Target(0, p.value, p.value, 0.0, 0.0)
    tg = Target(KIND, p.value, p.value, 32.0, 2.0)  # C = 2, p = 2: d = 3
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
        nf.noncentred(object(), make_target(nf, *of.arrays(2, 3, 33), 2))


def test_realnvp_fullrank_and_preconditioned_get_past_every_refusal(nf):
    """the ELBO entry points get past every refusal that comes before device work and stop at the stand-in context's device ordinal (a
    positive HIP error code); the graph form is never an argument error"""
    from normalizingflows_jl_amd._lib import NF_KIND, FlowDesc, Target

    lib = nf.load_library()
    keep = (C.c_char * 4096)()
    C.cast(keep, C.POINTER(C.c_int32))[0] = 1 << 20  # no such device
    ctx = C.cast(keep, C.c_void_p)
    buf = (C.c_double * 256)()
    p = C.cast(buf, C.c_void_p)
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
            got = _five(lib, ctx, p, val, desc, Target(KIND, p.value, p.value, 64.0, 4.0))  # C = 4, p = 4: d = 7
            assert all(c > 0 for c in got[:4]) and (got[4] > 0 or got[4] == -2), (kind, dtype, got)


# ---- host packing -------------------------------------------------------------------------------------------------------------------
def test_host_packing_is_sorted_blocked_and_padded_with_zero_weights(nf):
    """(5, 4, 70) with category 3 emptied: R is the sum of the labels' whole blocks, every block holds one label in ascending order, the
    caller's rows keep their order inside a label, padding rows are all zero with weight exactly 0, n_k are the weight sums (0 for the
    empty category, which has no block), the constants are folded -- and all of it equals the packing written directly"""
    Cn, p, rows = 5, 4, 70
    X, lab, off, wt = of.arrays(Cn, p, rows)
    lab = np.where(lab == 3, 1, lab)
    assert rows % 32 != 0 and (lab == 3).sum() == 0
    tgt = make_target(nf, X, lab, off, wt, Cn, const=0.25)
    Xd, p0 = of.target_arrays(tgt)
    counts = np.bincount(lab, minlength=Cn)
    R = int((32 * ((counts + 31) // 32)).sum())
    assert tgt.rows == rows and tgt.padded_rows == R == Xd.shape[0] and tgt.d == p + Cn - 1 and tgt.p == p and tgt.C == tgt.n_categories == Cn
    assert tgt.c.kind == KIND and tgt.c.s0 == R and tgt.c.s1 == Cn and tgt.c.p0 == tgt.p0.data_ptr() and tgt.c.p1 == tgt.A.data_ptr()
    o_, w_, bl, par, nk = of.split_p0(p0, R, Cn)
    assert (np.diff(bl) >= 0).all() and 3.0 not in bl and set(bl) == {0.0, 1.0, 2.0, 4.0}
    assert [int((bl == k).sum()) for k in range(Cn)] == list((counts + 31) // 32)
    k = np.repeat(bl.astype(int), 32)
    row = 0
    for c in range(Cn):
        idx = np.nonzero(lab == c)[0]  # ascending: the stable order
        blockrows = np.nonzero(k == c)[0]
        assert np.array_equal(Xd[blockrows[:len(idx)]], X[idx]) and np.array_equal(o_[blockrows[:len(idx)]], off[idx])
        assert np.array_equal(w_[blockrows[:len(idx)]], wt[idx])
        pad = blockrows[len(idx):]
        assert not Xd[pad].any() and not o_[pad].any() and (w_[pad] == 0.0).all() and not np.signbit(w_[pad]).any()
        row += len(blockrows)
    assert row == R
    assert np.array_equal(nk, [wt[lab == c].sum() for c in range(Cn)]) and nk[3] == 0.0
    want = 0.25 - 0.5 * p * math.log(2 * math.pi * of.SIGMA_BETA**2) - 0.5 * (Cn - 1) * math.log(2 * math.pi * of.SIGMA_CUT**2)
    assert par[0] == 1 / of.SIGMA_BETA**2 and par[2] == 1 / of.SIGMA_CUT**2 and par[3] == of.CUT_LOC and abs(par[1] - want) <= 1e-14 * abs(want)
    Xw, pw = of.pack(X, lab, off, wt, Cn, const=0.25)
    assert np.array_equal(Xd, Xw) and np.allclose(p0, pw, rtol=1e-15, atol=0)
    assert np.array_equal(tgt.order.numpy(), np.argsort(lab, kind="stable")) and np.array_equal(Xd[tgt.row_index.numpy()], X[tgt.order.numpy()])
    # the flat priors, defaults, Float32, labels as floats of X's type
    flat = nf.OrdinalRegressionTarget(_t(X), torch.tensor(lab), Cn, prior_sigma=math.inf, cut_sigma=math.inf)
    pf = of.split_p0(flat.p0.numpy(), R, Cn)
    assert list(pf[3]) == [0.0, 0.0, 0.0, 0.0] and (pf[1][np.repeat(pf[2], 32) >= 0].sum() == rows) and np.array_equal(pf[4], counts)
    t32 = nf.OrdinalRegressionTarget(_t(X, torch.float32), _t(lab, torch.float32), float(Cn))
    assert t32.A.dtype == torch.float32 and t32.p0.dtype == torch.float32 and t32.n_categories == Cn
    exact = make_target(nf, X[:64], np.arange(64) % 2, off[:64], wt[:64], 2)  # whole blocks: nothing is padded
    assert exact.padded_rows == 64


def test_constructor_refuses_bad_arguments(nf):
    E = nf.NFHipError
    X, lab, off, wt = of.arrays(5, 4, 70)
    X, off, wt, lab = _t(X), _t(off), _t(wt), torch.tensor(lab)
    T = nf.OrdinalRegressionTarget
    bad = [
        lambda: T(X[0], lab, 5),                                   # not a matrix
        lambda: T(X.to(torch.float16), lab, 5),
        lambda: T(X * math.inf, lab, 5),
        lambda: T(X, lab, 1),
        lambda: T(X, lab, 17),
        lambda: T(X, lab, 4),                                      # a label of 4 with four categories
        lambda: T(X, lab, 2.5),
        lambda: T(X, lab, True),
        lambda: T(X, lab, "5"),
        lambda: T(X, lab[:-1], 5),
        lambda: T(X, lab - 1, 5),                                  # a negative label
        lambda: T(X, lab.double() + 0.5, 5),                       # not integers
        lambda: T(X, lab.float(), 5),                              # element types differ
        lambda: T(X, lab.double() * math.nan, 5),
        lambda: T(torch.ones(40, 255, dtype=torch.float64), torch.zeros(40, dtype=torch.int64), 3),   # d = 257
        lambda: T(torch.ones(40, 242, dtype=torch.float64), torch.zeros(40, dtype=torch.int64), 16),  # d = 257
        lambda: T(X, lab, 5, offset=off[:-1]),
        lambda: T(X, lab, 5, offset=off * math.inf),
        lambda: T(X, lab, 5, offset=off.float()),
        lambda: T(X, lab, 5, offset=off.to("meta")),               # devices differ
        lambda: T(X, lab, 5, weights=-wt - 1),
        lambda: T(X, lab, 5, weights=wt[:-1]),
        lambda: T(X, lab, 5, prior_sigma=0.0),
        lambda: T(X, lab, 5, prior_sigma=-math.inf),
        lambda: T(X, lab, 5, prior_sigma=math.nan),
        lambda: T(X, lab, 5, cut_sigma=0.0),
        lambda: T(X, lab, 5, cut_sigma=math.nan),
        lambda: T(X, lab, 5, cut_loc=math.inf),
        lambda: T(X, lab, 5, cut_loc=math.nan),
        lambda: T(X, lab, 5, const=math.nan),
        lambda: T(X, lab, 5, const=math.inf),
    ]
    for i, make in enumerate(bad):
        with pytest.raises(E):
            make()
            pytest.fail(f"case {i} was accepted")
    T(torch.ones(40, 255, dtype=torch.float64), torch.arange(40) % 2, 2)     # d = 256
    T(torch.ones(40, 241, dtype=torch.float64), torch.arange(40) % 16, 16)   # d = 256
    T(X, lab, 16)                                                            # categories without rows
    T(X, lab, 5, weights=torch.zeros(70, dtype=torch.float64))


def test_unpack_and_predict(nf):
    Cn, p, rows = 5, 4, 70
    X, lab, off, wt = of.arrays(Cn, p, rows)
    tgt = make_target(nf, X, lab, off, wt, Cn)
    ys = of.sample_ys(Cn, p, 6, 0.5)
    c_ref, _ = of.cutpoints(ys[p:])
    beta, cut = tgt.unpack(_t(ys[:, 0]))
    assert beta.shape == (p,) and cut.shape == (Cn - 1,) and np.array_equal(beta.numpy(), ys[:p, 0])
    assert np.allclose(cut.numpy(), c_ref[:, 0], rtol=1e-15, atol=0) and (np.diff(cut.numpy()) > 0).all()
    bb, cb = tgt.unpack(_t(ys))
    assert bb.shape == (p, 6) and cb.shape == (Cn - 1, 6) and np.allclose(cb.numpy(), c_ref, rtol=1e-15, atol=0)
    Xn = np.random.default_rng(0).standard_normal((9, p))
    pr = tgt.predict(_t(ys), _t(Xn)).numpy()
    assert pr.shape == (Cn, 9, 6) and np.allclose(pr.sum(0), 1.0, rtol=0, atol=1e-14) and (pr > 0).all()
    sig = lambda u: 1 / (1 + np.exp(-u))
    eta = Xn @ ys[:p]
    cdf = np.concatenate([np.zeros((1, 9, 6)), sig(c_ref[:, None, :] - eta[None]), np.ones((1, 9, 6))])
    assert np.allclose(pr, np.diff(cdf, axis=0), rtol=0, atol=1e-14)
    assert np.allclose(tgt.predict(_t(ys[:, 2]), _t(Xn)).numpy(), pr[:, :, 2], rtol=0, atol=1e-14)
    o9 = np.linspace(-1, 1, 9)
    assert np.allclose(tgt.predict(_t(ys), _t(Xn), offset=_t(o9)).numpy(), np.diff(np.concatenate(
        [np.zeros((1, 9, 6)), sig(c_ref[:, None, :] - (eta + o9[:, None])[None]), np.ones((1, 9, 6))]), axis=0), rtol=0, atol=1e-14)
    # the likelihood part of log p is the sum of the weighted log-probabilities predict gives for the data's own rows
    prd = tgt.predict(_t(ys), _t(X), offset=_t(off)).numpy()
    lik = (wt[:, None] * np.log(prd[lab, np.arange(rows)])).sum(0)
    flat = make_target(nf, X, lab, off, wt, Cn, prior_sigma=math.inf, cut_sigma=math.inf)
    got = of.ref_of(flat)(ys)[0] - ys[p + 1:].sum(0)
    assert np.allclose(got, lik, rtol=1e-12, atol=0)
    for bad in (lambda: tgt.unpack(_t(ys[:-1])), lambda: tgt.predict(_t(ys), _t(Xn[:, :1])), lambda: tgt.predict(_t(ys), _t(Xn[0]))):
        with pytest.raises(nf.NFHipError):
            bad()


def test_check_compatible_and_builtin_routing(nf):
    from normalizingflows_jl_amd import objectives as ob
    from normalizingflows_jl_amd.flows import check_target

    X, lab, off, wt = of.arrays(5, 4, 70)
    t = make_target(nf, X, lab, off, wt, 5, torch.float32)
    assert t.d == 8 and isinstance(t, ob._BUILTIN) and isinstance(t, ob._LINPRED)
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


# ---- the numpy form -----------------------------------------------------------------------------------------------------------------
def _case(shape, gscale, n):
    Cn, p, rows = shape
    X, lab, off, wt = of.arrays(*shape)
    Xp, p0 = of.pack(X, lab, off, wt, Cn)
    return Xp, p0, of.sample_ys(Cn, p, n, gscale)


@pytest.mark.parametrize("gscale", of.GAMMA_SCALES)
@pytest.mark.parametrize("shape", [(2, 3, 33), (5, 4, 70), (16, 6, 133)], ids=lambda s: "C%d_p%d_r%d" % s)
def test_the_form_is_the_derivative_of_its_value(shape, gscale):
    """central differences in float64, every coordinate of beta and gamma: the value's differences agree with the score to 1e-6 of
    max(1, |score|) (the step is 1e-5 relative to 1 + |y_i|: truncation 1e-10 |f'''|, round-off 1e-16 |f| / 1e-5)"""
    Cn, p, rows = shape
    Xp, p0, y0 = _case(shape, gscale, 1)
    sc = of.logp_score(y0, Xp, p0, Cn)[1][:, 0]
    worst = 0.0
    for i in range(y0.shape[0]):
        e = np.zeros_like(y0)
        e[i] = 1e-5
        fd = (of.logp_score(y0 + e, Xp, p0, Cn)[0][0] - of.logp_score(y0 - e, Xp, p0, Cn)[0][0]) / 2e-5
        worst = max(worst, abs(fd - sc[i]) / max(1.0, abs(sc[i])))
    print(f"ordinal central differences {shape} gamma x{gscale}: {worst:.2e}")
    assert worst <= 1e-6, (shape, gscale, worst)


@pytest.mark.parametrize("gscale", of.GAMMA_SCALES)
@pytest.mark.parametrize("shape", [(2, 3, 33), (5, 4, 70), (5, 30, 40), (16, 6, 133)], ids=lambda s: "C%d_p%d_r%d" % s)
def test_the_factored_form_is_the_unfactored_definition(shape, gscale):
    """log(sigmoid(a) - sigmoid(b)) summed row by row (50 digits where mpmath is importable) against the factored float64 form:
    at most 1e-12 relative"""
    Cn, p, rows = shape
    Xp, p0, ys = _case(shape, gscale, 3)
    if of.mpmath is None:
        c, _ = of.cutpoints(ys[p:])
        assert np.abs(c).max() + np.abs(Xp @ ys[:p]).max() + 1.0 <= 30.0
    got = of.logp_score(ys, Xp, p0, Cn)[0]
    want = of.unfactored_logp(ys, Xp, p0, Cn)
    rel = np.abs(got - want) / np.abs(want)
    print(f"ordinal factored vs unfactored {shape} gamma x{gscale}: {rel.max():.2e} ({'mpmath' if of.mpmath else 'float64'})")
    assert np.isfinite(want).all() and rel.max() <= 1e-12, (shape, gscale, rel)


def test_two_categories_are_logistic_regression_on_the_extended_design():
    """C = 2: P(k = 1) = sigmoid(eta - c_1), so log p is glm_forms' logit regression on A = s [X, -1], off' = s off (s = +-1 by label)
    with y = [beta ; c_1] -- under flat priors, and with both ordinal priors N(0, sigma^2), the GLM's isotropic prior over its
    d = p + 1 coordinates (normalisers included); value and score"""
    Cn, p, rows = 2, 3, 33
    X, lab, off, wt = of.arrays(Cn, p, rows)
    ys = of.sample_ys(Cn, p, 7, 2.0)
    s = 2.0 * lab - 1.0
    A = s[:, None] * np.hstack([X, -np.ones((rows, 1))])
    glm_p0 = np.concatenate([np.zeros(p + 1), s * off, wt, [0.0, 0.0]])
    for sigma in (np.inf, 2.0):
        Xp, p0 = of.pack(X, lab, off, wt, Cn, sigma_beta=sigma, sigma_cut=sigma, cut_loc=0.0)
        got = of.logp_score(ys, Xp, p0, Cn)
        want = gf.logp_score("logit", ys, A, glm_p0, sigma)
        assert np.allclose(got[0], want[0], rtol=1e-13, atol=0) and np.abs(got[1] - want[1]).max() <= 1e-13 * np.abs(want[1]).max(), sigma


def test_a_zero_weight_row_of_huge_features_leaves_the_form_alone():
    Cn, p, rows = 5, 4, 70
    X, lab, off, wt = of.arrays(Cn, p, rows)
    ys = of.sample_ys(Cn, p, 5, 2.0)
    want = of.logp_score(ys, *of.pack(X, lab, off, wt, Cn), Cn)
    Xb, pb = of.pack(np.vstack([X, np.full((1, p), 1e30)]), np.append(lab, 2), np.append(off, 50.0), np.append(wt, 0.0), Cn)
    assert Xb.shape[0] == of.pack(X, lab, off, wt, Cn)[0].shape[0]  # the row took a padding slot of its label
    got = of.logp_score(ys, Xb, pb, Cn)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


# ---- the float32 floor of the GPU tests' inputs -------------------------------------------------------------------------------------
@pytest.mark.parametrize("gscale", of.GAMMA_SCALES)
@pytest.mark.parametrize("shape", of.SHAPES, ids=lambda s: "C%d_p%d_r%d" % s)
def test_the_float32_form_alone_stays_inside_the_tolerances(nf, shape, gscale):
    """the float32 form against the float64 one on the GPU tests' inputs, read back from the Float32 target the constructor folds (what
    the device reads): at most 0.5x the element-wise tolerance on log p and 0.5x GRAD_RTOL on the score, so the floor is not expected
    to decide a nf_target_logp check.  (Float32's unit round-off is 6e-8: a sum of a few hundred terms of either sign stays well below
    1e-5 relative; the fraction is a bound on how much of the tolerance the format itself may use, not a measurement.)"""
    Cn, p, rows = shape
    X, lab, off, wt = of.arrays(*shape)
    tgt = make_target(nf, X, lab, off, wt, Cn, torch.float32)
    Xd, p0 = of.target_arrays(tgt)
    Xw, pw = of.pack(X, lab, off, wt, Cn)
    assert np.array_equal(Xd, Xw) and np.allclose(p0, pw, rtol=1e-7, atol=0)
    for n in of.N_SIZES:
        ys = of.sample_ys(Cn, p, n, gscale)
        l64, s64 = of.logp_score(ys, Xd, p0, Cn)
        l32, s32 = of.logp_score(ys.astype(np.float32), Xd, p0, Cn)
        assert l32.dtype == s32.dtype == np.float32 and np.isfinite(l64).all() and np.isfinite(s64).all() and np.isfinite(s32).all()
        lr = float((np.abs(l32 - l64) / (P.Y_ATOL + P.Y_RTOL * np.abs(l64))).max())
        gr = float(np.abs(s32 - s64).max() / np.abs(s64).max()) / P.GRAD_RTOL
        print(f"ordinal floor {shape} gamma x{gscale:g} N={n}: logp {lr:.4f}x, score {gr:.5f}x")
        assert lr <= 0.5 and gr <= 0.5, (shape, gscale, n, lr, gr)


# ---- the float64 loop train_flow is compared with -----------------------------------------------------------------------------------
TRAIN = ((5, 4, 70), 64, 9, 0.05, 6)  # shape, draws, seed, Adam's rate, steps


def train_target(nf, device="cpu"):
    (Cn, p, rows) = TRAIN[0]
    X, lab, off, wt = of.arrays(Cn, p, rows)
    to = lambda a: torch.tensor(a, dtype=torch.float64, device=device)
    return nf.OrdinalRegressionTarget(to(X), torch.tensor(lab, device=device), Cn, offset=to(off), weights=to(wt), prior_sigma=of.SIGMA_BETA,
                                      cut_sigma=of.SIGMA_CUT, cut_loc=of.CUT_LOC)


def fullrank_numpy_losses(Xd, p0, Cn, n, seed, lr, iters, fixed=None):
    """Full-rank Gaussian VI on the ordinal posterior as a float64 numpy loop from theta = [0 ; I] (tests/fullrank_ref.py's layout):
    draws of stream i, the form's score, oracle Adam.  Returns the losses, theta, and -ELBO on the fixed draws before and after."""
    import fullrank_ref as fr
    import nf_oracle as o

    d = of.dim(Cn, Xd.shape[1])
    ref = lambda y: of.logp_score(y, Xd, p0, Cn)
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

    (Cn, p, rows), n, seed, lr, iters = TRAIN
    Xd, p0 = of.target_arrays(train_target(nf))
    fixed = o.base_sample(of.dim(Cn, p), 256, 1234, 0, 0, precision="f64")
    losses, th, before, after = fullrank_numpy_losses(Xd, p0, Cn, n, seed, lr, iters, fixed)
    print("ordinal fullrank numpy loop", losses, before, after)
    assert all(np.isfinite(losses)) and np.isfinite(th).all() and after < before


# ---- resources and sources -----------------------------------------------------------------------------------------------------------
def test_ordinal_kernels_use_no_scratch_and_fit_their_launch_bounds(nf):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources

    rows = kernel_resources.kernel_table(os.path.join(ROOT, "normalizingflows.jl_amd", "build"))
    assert len(rows) > 200, "the objects' metadata notes were not readable"
    for prefix, count in (("void k_target_ordinal_tiled<", 4), ("void k_target_ordinal<", 2)):  # DB in {1, 2, 4, 8}; {float, double}
        hit = [r for r in rows if r[0].startswith(prefix)]
        assert len(hit) == count, (prefix, [r[0][:60] for r in hit])
        for name, agpr, vgpr, sgpr, scratch, lds in hit:
            assert scratch == 0, (name, scratch)
            assert vgpr <= 512, (name, vgpr)    # 256 threads per workgroup: one wave per SIMD may use the whole register file
            assert lds <= 24576, (name, lds)    # static LDS: cutpoints, the d c slots and the reductions (the tile and the images are dynamic)
            if re.search(r"tiled<[12]>\(", name[:80]):
                assert vgpr <= 256, (name, vgpr)  # DB <= 2: two workgroups per CU


def test_the_new_source_is_built_and_has_no_build_time_variants():
    from __graft_entry__ import SOURCES

    assert "nf_ordinal.hip" in SOURCES
    src = open(os.path.join(ROOT, "normalizingflows.jl_amd", "csrc", "nf_ordinal.hip")).read()
    assert not re.search(r"^\s*#\s*if(def|ndef)?\b.*\bNF_", src, re.M)
    assert 'ProfScope ps(ctx, "target_ordinal")' in src
