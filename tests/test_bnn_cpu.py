"""CPU checks of the one-hidden-layer Bayesian neural-network targets (NF_TARGET_BNN_*, kinds 22..26): the constants (header,
Python mirror, Julia extension), nf_target_check's argument conventions as nf_target_logp reports them BEFORE any device work (a
stand-in context is enough), the refusals of the flows that evaluate their target in their own kernels, the descriptors that get
past every refusal, the constructors' float64 folding against the model written directly with scipy, the three conveniences
against BNNTarget, the constructors' refusals, unpack / predict, the routing of the Python mirror, the numpy form against central
differences, the float32 floor of the GPU tests' inputs, the float64 training loop test_gpu_bnn.py compares train_flow with, and
the new kernels' resources."""
import ctypes as C
import math
import os
import re
import sys

import numpy as np
import pytest
import torch
from scipy import special as sp
from scipy import stats

import bnn_forms as bf
import parity as P
from __graft_entry__ import ROOT, build, load_package

BNN_KINDS = {"logit": 22, "probit": 23, "poisson": 24, "student": 25, "normal": 26}


@pytest.fixture(scope="module")
def nf():
    build()  # no-op when libnfhip.so is up to date
    return load_package()


def _standin():
    return C.cast((C.c_char * 4096)(), C.c_void_p)


def _t(a):
    return torch.tensor(np.asarray(a), dtype=torch.float64)


def test_constants_match_the_header_the_mirror_and_the_julia_extension(nf):
    hdr = open(os.path.join(ROOT, "include", "nfhip.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"^#define (NF_TARGET_\w+) (\d+)", hdr, re.M)}
    jl = open(os.path.join(ROOT, "ext", "NormalizingFlowsNFHipExt.jl")).read()
    m = re.search(r"const NF_TARGET_BNN_LOGIT, NF_TARGET_BNN_PROBIT, NF_TARGET_BNN_POISSON, NF_TARGET_BNN_STUDENT, NF_TARGET_BNN_NORMAL =\s*"
                  r"Int32\((\d+)\), Int32\((\d+)\), Int32\((\d+)\), Int32\((\d+)\), Int32\((\d+)\)", jl)
    assert m, "the Julia extension does not define the five constants"
    assert [int(x) for x in m.groups()] == [22, 23, 24, 25, 26]
    for fam, v in BNN_KINDS.items():
        name = "NF_TARGET_BNN_" + fam.upper()
        assert defs[name] == getattr(nf._lib, name) == v == defs["NF_TARGET_GLM_" + fam.upper()] + 13
        assert re.search(r":%s => %s\b" % (fam, name), jl), name
    for name, v in defs.items():
        assert getattr(nf._lib, name) == v
    mirror = [v for k, v in vars(nf._lib).items() if k.startswith("NF_TARGET_")]
    for absent in (7, 14, 21, 27):
        assert absent not in defs.values() and absent not in mirror
    from normalizingflows_jl_amd import flows

    assert flows._BNN_KINDS == BNN_KINDS
    assert nf.load_library().nf_abi_version() == 4


def test_target_check_errors_come_before_device_work(nf):
    """NF_ERR_ARG (-1) and NF_ERR_UNSUPPORTED (-2) for every violated convention of kinds 22..26 without touching the context
    (N = 0: nothing is launched, and a good target's answer is no error)"""
    from normalizingflows_jl_amd._lib import Target

    lib = nf.load_library()
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p).value
    ctx = _standin()

    def logp(t, d=7, n=4, dtype=0):
        return lib.nf_target_logp(ctx, dtype, C.byref(t), d, n, C.c_void_p(p), C.c_void_p(p), None)

    for kind in BNN_KINDS.values():
        for dtype in (0, 1):
            assert logp(Target(kind, 0, p, 8.0, 2.0), dtype=dtype) == -1             # p0 = NULL
            assert logp(Target(kind, p, 0, 8.0, 2.0), dtype=dtype) == -1             # p1 = NULL
            assert logp(Target(kind, p, p, 0.0, 2.0), dtype=dtype) == -1             # rows = 0
            assert logp(Target(kind, p, p, -3.0, 2.0), dtype=dtype) == -1            # negative rows
            assert logp(Target(kind, p, p, 2.5, 2.0), dtype=dtype) == -1             # rows not integral
            assert logp(Target(kind, p, p, 2147483648.0, 2.0), dtype=dtype) == -1    # rows = 2^31
            assert logp(Target(kind, p, p, math.nan, 2.0), dtype=dtype) == -1        # NaN rows
            assert logp(Target(kind, p, p, 8.0, 0.0), dtype=dtype) == -1             # H = 0
            assert logp(Target(kind, p, p, 8.0, -2.0), dtype=dtype) == -1            # negative H
            assert logp(Target(kind, p, p, 8.0, 17.0), d=52, dtype=dtype) == -1      # H = 17 (d = 17 * 3 + 1)
            assert logp(Target(kind, p, p, 8.0, 1.5), dtype=dtype) == -1             # H not integral
            assert logp(Target(kind, p, p, 8.0, math.nan), dtype=dtype) == -1        # NaN H
            assert logp(Target(kind, p, p, 8.0, math.inf), dtype=dtype) == -1
            assert logp(Target(kind, p, p, 8.0, 4.0), dtype=dtype) == -1             # (d - 1) % H != 0 (6 % 4)
            assert logp(Target(kind, p, p, 8.0, 2.0), d=8, dtype=dtype) == -1        # (d - 1) % H != 0 (7 % 2)
            assert logp(Target(kind, p, p, 8.0, 6.0), dtype=dtype) == -1             # d = H + 1: p = 0
            assert logp(Target(kind, p, p, 8.0, 1.0), d=2, dtype=dtype) == -1        # d < H + 2
            assert logp(Target(kind, p, p, 8.0, 3.0), d=4, dtype=dtype) == -1        # d = H + 1
            assert logp(Target(kind, p, p, 8.0, 1.0), d=1, dtype=dtype) == -1
            assert logp(Target(kind, p, p, 8.0, 3.0), d=258, dtype=dtype) == -1      # 257 % 3 != 0: an argument error first
            assert logp(Target(kind, p, p, 8.0, 2.0), d=257, dtype=dtype) == -2      # d = 257 (H = 2, p = 127)
            assert logp(Target(kind, p, p, 8.0, 16.0), d=257, dtype=dtype) == -2     # d = 257 (H = 16, p = 15)
            assert logp(Target(kind, p, p, 8.0, 1.0), d=131, dtype=dtype) == -2      # p = 129
            assert logp(Target(kind, p, p, 8.0, 1.0), d=256, dtype=dtype) == -2      # p = 254: one image does not fit
            assert logp(Target(kind, p, p, 8.0, 1.0), d=257, n=0, dtype=dtype) == -2
            assert logp(Target(kind, p, p, 8.0, 2.0), n=0, dtype=dtype) >= 0         # past the check (H = 2, p = 2)
            assert logp(Target(kind, p, p, 8.0, 1.0), d=3, n=0, dtype=dtype) >= 0    # the smallest: H = 1, p = 1
            assert logp(Target(kind, p, p, 8.0, 16.0), d=241, n=0, dtype=dtype) >= 0  # H at its cap
            assert logp(Target(kind, p, p, 8.0, 1.0), d=130, n=0, dtype=dtype) >= 0  # p at its cap
            assert logp(Target(kind, p, p, 8.0, 3.0), d=256, n=0, dtype=dtype) >= 0  # d at its cap (p = 84)
            assert logp(Target(kind, p, p, 2147483647.0, 2.0), n=0, dtype=dtype) >= 0
    for absent in (7, 14, 21, 27, 28):
        assert logp(Target(absent, p, p, 8.0, 2.0)) == -1  # no such kinds


def _five(lib, ctx, p, val, desc, tgt):
    return [lib.nf_elbo_value_and_grad(ctx, C.byref(desc), C.byref(tgt), p, p, 8, 8, 1, 0, 0, p),
            lib.nf_elbo_batch(ctx, C.byref(desc), C.byref(tgt), p, p, 8, None, C.byref(val)),
            lib.nf_elbo_batch_rng(ctx, C.byref(desc), C.byref(tgt), p, 8, 1, 0, 0, C.byref(val)),
            lib.nf_elbo_step(ctx, C.byref(desc), C.byref(tgt), p, p, p, 8, 1, 0, 1e-3, 0.9, 0.999, 1e-8, None, None),
            lib.nf_elbo_step_enqueue(ctx, C.byref(desc), C.byref(tgt), p, p, p, 8, 1, p, 1e-3, 0.9, 0.999, 1e-8, None)]


def test_flows_that_evaluate_the_target_in_their_own_kernels_refuse_before_device_work(nf):
    """planar, radial, mean-field and Hamiltonian descriptors answer NF_ERR_UNSUPPORTED (-2) at all five ELBO entry points, with a
    network kind as the target and as the Hamiltonian score -- the stand-in context is never used."""
    from normalizingflows_jl_amd._lib import NF_KIND, FlowDesc, Target

    lib = nf.load_library()
    buf = (C.c_double * 256)()
    p = C.cast(buf, C.c_void_p)
    ctx = _standin()
    val = C.c_double(0.0)
    diag = Target(0, p.value, p.value, 0.0, 0.0)
    for tk in BNN_KINDS.values():
        bn = Target(tk, p.value, p.value, 4.0, 1.0)  # H = 1, p = 1: d = 3
        for kind, dtype in (("planar", 0), ("radial", 0), ("meanfield", 1), ("planar", 1)):
            desc = FlowDesc()
            desc.kind, desc.dtype, desc.d, desc.nlayers = NF_KIND[kind], dtype, 3, 2
            assert _five(lib, ctx, p, val, desc, bn) == [-2] * 5, (kind, tk)
        hd = FlowDesc()
        hd.kind, hd.dtype, hd.d, hd.nlayers, hd.K = NF_KIND["hamiltonian"], 0, 6, 2, 3
        hd.score = C.cast(C.pointer(diag), C.c_void_p)  # a supported score, a network ELBO target
        assert _five(lib, ctx, p, val, hd, bn) == [-2] * 5, tk
        hd.score = C.cast(C.pointer(bn), C.c_void_p)    # a network score
        assert _five(lib, ctx, p, val, hd, diag) == [-2] * 5, tk


def test_realnvp_fullrank_and_preconditioned_get_past_every_refusal(nf):
    """RealNVP, full-rank and preconditioned descriptors of either element type with a network kind: the ELBO entry points get past
    every refusal that comes before device work and stop at the stand-in context's device ordinal (a positive HIP error code);
    the graph form is never an argument error (its NF_ERR_UNSUPPORTED may come before or after the device ordinal)"""
    from normalizingflows_jl_amd._lib import NF_KIND, FlowDesc, Target

    lib = nf.load_library()
    keep = (C.c_char * 4096)()
    C.cast(keep, C.POINTER(C.c_int32))[0] = 1 << 20  # no such device
    ctx = C.cast(keep, C.c_void_p)
    buf = (C.c_double * 256)()
    p = C.cast(buf, C.c_void_p)
    val = C.c_double(0.0)

    def coupling(dtype):
        desc = FlowDesc()
        desc.kind, desc.dtype, desc.d, desc.nlayers, desc.n_hidden = NF_KIND["realnvp"], dtype, 7, 2, 2
        desc.hdims[0] = desc.hdims[1] = 32
        return desc

    for kind in ("realnvp", "fullrank", "preconditioned"):
        for dtype in (0, 1):
            inner = coupling(dtype)
            if kind == "realnvp":
                desc = inner
            else:
                desc = FlowDesc()
                desc.kind, desc.dtype, desc.d, desc.nlayers = NF_KIND[kind], dtype, 7, 1
                if kind == "preconditioned":
                    desc.nsegments = 1
                    desc.segments = C.cast(C.pointer(inner), C.c_void_p)
            for tk in BNN_KINDS.values():
                got = _five(lib, ctx, p, val, desc, Target(tk, p.value, p.value, 4.0, 2.0))  # H = 2, p = 2: d = 7
                assert all(c > 0 for c in got[:4]) and (got[4] > 0 or got[4] == -2), (kind, dtype, tk, got)


# ---- host folding ---------------------------------------------------------------------------------------------------------------
HID, PF, ROWS, NB = 3, 2, 7, 5
D = HID * (PF + 1) + 1


def _data(seed=0):
    g = np.random.default_rng(seed)
    X = g.standard_normal((ROWS, PF)) / np.sqrt(PF)
    X[:, 0] = 1.0
    w = g.uniform(0.3, 2.5, ROWS)
    w[2] = 0.0  # one dropped row
    ys = g.standard_normal((D, NB))
    return g, X, w, ys


def _network(X, ys):
    """f [rows, N] written directly: W [p, H] per sample"""
    out = np.empty((X.shape[0], ys.shape[1]))
    for n in range(ys.shape[1]):
        W = ys[:HID * PF, n].reshape(HID, PF).T
        out[:, n] = np.tanh(X @ W) @ ys[HID * PF:HID * PF + HID, n] + ys[-1, n]
    return out


def _prior(ys, sh, so):
    return stats.norm.logpdf(ys[:HID * PF], 0.0, sh).sum(0) + stats.norm.logpdf(ys[HID * PF:], 0.0, so).sum(0)


def _folded(tgt, ys):
    return bf.ref_of(tgt)(ys)[0]


def _close(got, want):
    assert got.shape == want.shape and (np.abs(got - want) <= 1e-12 * np.abs(want)).all(), (got, want)


def test_bnn_target_folding_against_the_model_written_directly(nf):
    g, X, w, ys = _data(1)
    f = _network(X, ys)
    scl, off = g.uniform(0.5, 2.0, ROWS) * g.choice([-1.0, 1.0], ROWS), 0.4 * g.standard_normal(ROWS)
    u = scl[:, None] * f + off[:, None]
    lik = {"logit": stats.bernoulli.logpmf(1, sp.expit(u)), "probit": stats.norm.logcdf(u), "poisson": -np.exp(u),
           "student": -0.5 * (3.5 + 1.0) * np.log1p(u * u / 3.5), "normal": -0.5 * u * u}
    for fam, ll in lik.items():
        tgt = nf.BNNTarget(fam, _t(X), HID, scale=_t(scl), offset=_t(off), weights=_t(w), const=0.25, param=3.5 if fam == "student" else None,
                           prior_sigma_hidden=1.7, prior_sigma_out=0.6)
        _close(_folded(tgt, ys), 0.25 + (w[:, None] * ll).sum(0) + _prior(ys, 1.7, 0.6))
        assert tgt.d == D and tgt.p == PF and tgt.n_hidden == HID and tgt.rows == ROWS and tgt.family == fam
        assert tgt.A.dtype == torch.float64 and tgt.p0.dtype == torch.float64 and tgt.p0.shape == (3 * ROWS + 4,)
        assert tgt.c.kind == BNN_KINDS[fam] and tgt.c.p0 == tgt.p0.data_ptr() and tgt.c.p1 == tgt.A.data_ptr() and tgt.c.s0 == ROWS and tgt.c.s1 == HID
        assert float(tgt.p0[-2]) == 1.0 / 1.7**2 and float(tgt.p0[-1]) == 1.0 / 0.6**2 and float(tgt.p0[-4]) == (3.5 if fam == "student" else 0.0)
        assert np.allclose(tgt.p0.numpy(), bf.p0_of(scl, off, w, float(tgt.p0[-4]), HID, PF, 1.7, 0.6, 0.25), rtol=1e-15, atol=0)
    # defaults, the flat priors one at a time, Float32
    plain = nf.BNNTarget("normal", _t(X), HID)
    assert torch.equal(plain.p0[:3 * ROWS], torch.cat([torch.ones(ROWS), torch.zeros(ROWS), torch.ones(ROWS)]).double())
    _close(_folded(plain, ys), (-0.5 * f * f).sum(0) + _prior(ys, 1.0, 1.0))
    fh = nf.BNNTarget("normal", _t(X), HID, prior_sigma_hidden=math.inf)
    assert float(fh.p0[-2]) == 0.0 and float(fh.p0[-1]) == 1.0
    _close(_folded(fh, ys), (-0.5 * f * f).sum(0) + stats.norm.logpdf(ys[HID * PF:], 0.0, 1.0).sum(0))
    fo = nf.BNNTarget("normal", _t(X), HID, prior_sigma_hidden=math.inf, prior_sigma_out=math.inf)
    assert float(fo.p0[-1]) == 0.0 and float(fo.p0[-3]) == 0.0
    _close(_folded(fo, ys), (-0.5 * f * f).sum(0))
    t32 = nf.BNNTarget("logit", _t(X).float(), HID, weights=_t(w).float())
    assert t32.A.dtype == torch.float32 and t32.p0.dtype == torch.float32
    same = nf.BNNTarget("normal", _t(X), float(HID))
    assert torch.equal(same.p0, plain.p0) and same.n_hidden == HID


def test_the_three_conveniences_against_scipy_and_bnn_target(nf):
    g, X, w, ys = _data(2)
    f = _network(X, ys)
    t = g.standard_normal(ROWS)
    reg = nf.BNNRegressionTarget(_t(X), _t(t), HID, noise_sigma=0.7, weights=_t(w), prior_sigma_hidden=2.0, prior_sigma_out=1.5)
    _close(_folded(reg, ys), (w[:, None] * stats.norm.logpdf(t[:, None], f, 0.7)).sum(0) + _prior(ys, 2.0, 1.5))
    const = float(w.sum()) * (-0.5 * math.log(2.0 * math.pi) - math.log(0.7))
    direct = nf.BNNTarget("normal", _t(X), HID, scale=_t(np.full(ROWS, 1.0 / 0.7)), offset=_t(-t / 0.7), weights=_t(w), const=const,
                          prior_sigma_hidden=2.0, prior_sigma_out=1.5)
    assert isinstance(reg, nf.BNNTarget) and reg.family == "normal" and torch.equal(reg.p0, direct.p0) and torch.equal(reg.A, direct.A)
    rob = nf.BNNRegressionTarget(_t(X), _t(t), HID, noise_sigma=0.7, nu=4.0, weights=_t(w))
    _close(_folded(rob, ys), (w[:, None] * stats.t.logpdf(t[:, None], 4.0, loc=f, scale=0.7)).sum(0) + _prior(ys, 1.0, 1.0))
    assert rob.family == "student" and rob.param == 4.0 and rob.c.kind == 25
    lab = g.integers(0, 2, ROWS)
    for link, cdf in (("logit", sp.expit), ("probit", stats.norm.cdf)):
        cls = nf.BNNClassifierTarget(_t(X), torch.tensor(lab), HID, link=link, weights=_t(w), prior_sigma_out=3.0)
        _close(_folded(cls, ys), (w[:, None] * stats.bernoulli.logpmf(lab[:, None], cdf(f))).sum(0) + _prior(ys, 1.0, 3.0))
        direct = nf.BNNTarget(link, _t(X), HID, scale=_t(2.0 * lab - 1.0), weights=_t(w), prior_sigma_out=3.0)
        assert cls.family == link and torch.equal(cls.p0, direct.p0)
        same = nf.BNNClassifierTarget(_t(X), _t(lab.astype(np.float64)), HID, link=link, weights=_t(w), prior_sigma_out=3.0)
        assert torch.equal(same.p0, cls.p0)


def test_constructors_refuse_bad_arguments(nf):
    E = nf.NFHipError
    g, X, w, _ = _data(3)
    X, w = _t(X), _t(w)
    lab = torch.tensor([0, 1, 1, 0, 1, 0, 1])
    tv = _t(g.standard_normal(ROWS))
    bad = [
        lambda: nf.BNNTarget("gamma", X, 3),                                         # no such family
        lambda: nf.BNNTarget("normal", X[0], 3),                                     # not a matrix
        lambda: nf.BNNTarget("normal", X.to(torch.float16), 3),
        lambda: nf.BNNTarget("normal", X * math.inf, 3),
        lambda: nf.BNNTarget("normal", X, 0),
        lambda: nf.BNNTarget("normal", X, 17),
        lambda: nf.BNNTarget("normal", X, -1),
        lambda: nf.BNNTarget("normal", X, 2.5),
        lambda: nf.BNNTarget("normal", X, True),
        lambda: nf.BNNTarget("normal", X, "3"),
        lambda: nf.BNNTarget("normal", torch.ones(4, 129, dtype=torch.float64), 1),  # p = 129
        lambda: nf.BNNTarget("normal", torch.ones(4, 127, dtype=torch.float64), 2),  # d = 257
        lambda: nf.BNNTarget("normal", torch.ones(4, 15, dtype=torch.float64), 16),  # d = 257
        lambda: nf.BNNTarget("normal", X, 3, scale=w[:-1]),
        lambda: nf.BNNTarget("normal", X, 3, scale=w * math.nan),
        lambda: nf.BNNTarget("normal", X, 3, scale=w.float()),                       # element types differ
        lambda: nf.BNNTarget("normal", X, 3, offset=w[:-1]),
        lambda: nf.BNNTarget("normal", X, 3, offset=w * math.inf),
        lambda: nf.BNNTarget("normal", X, 3, offset=w.to("meta")),                   # devices differ
        lambda: nf.BNNTarget("normal", X, 3, weights=-w),
        lambda: nf.BNNTarget("normal", X, 3, weights=w[:-1]),
        lambda: nf.BNNTarget("normal", X, 3, const=math.nan),
        lambda: nf.BNNTarget("normal", X, 3, const=math.inf),
        lambda: nf.BNNTarget("normal", X, 3, param=math.nan),
        lambda: nf.BNNTarget("student", X, 3),                                       # nu missing
        lambda: nf.BNNTarget("student", X, 3, param=0.0),
        lambda: nf.BNNTarget("student", X, 3, param=-2.0),
        lambda: nf.BNNTarget("normal", X, 3, prior_sigma_hidden=0.0),
        lambda: nf.BNNTarget("normal", X, 3, prior_sigma_hidden=-math.inf),
        lambda: nf.BNNTarget("normal", X, 3, prior_sigma_out=math.nan),
        lambda: nf.BNNTarget("normal", X, 3, prior_sigma_out=-1.0),
        lambda: nf.BNNRegressionTarget(X, tv[:-1], 3),
        lambda: nf.BNNRegressionTarget(X, tv * math.nan, 3),
        lambda: nf.BNNRegressionTarget(X, tv, 3, noise_sigma=0.0),
        lambda: nf.BNNRegressionTarget(X, tv, 3, noise_sigma=math.inf),
        lambda: nf.BNNRegressionTarget(X, tv, 3, nu=0.0),
        lambda: nf.BNNRegressionTarget(X, tv, 3, weights=-w),
        lambda: nf.BNNRegressionTarget(X, tv, 17),
        lambda: nf.BNNClassifierTarget(X, lab[:-1], 3),
        lambda: nf.BNNClassifierTarget(X, 2 * lab - 1, 3),                           # labels in {-1, +1}
        lambda: nf.BNNClassifierTarget(X, lab + 1, 3),
        lambda: nf.BNNClassifierTarget(X, lab.double() * 0.5, 3),
        lambda: nf.BNNClassifierTarget(X, lab.float(), 3),                           # element types differ
        lambda: nf.BNNClassifierTarget(X, lab, 3, link="cloglog"),
        lambda: nf.BNNClassifierTarget(X, lab, 0),
    ]
    for i, make in enumerate(bad):
        with pytest.raises(E):
            make()
            pytest.fail(f"case {i} was accepted")
    nf.BNNTarget("normal", torch.ones(4, 128, dtype=torch.float64), 1)               # p = 128, d = 130
    nf.BNNTarget("poisson", torch.ones(4, 14, dtype=torch.float64), 16, weights=torch.zeros(4, dtype=torch.float64))  # d = 241
    nf.BNNTarget("normal", torch.ones(4, 84, dtype=torch.float64), 3, prior_sigma_hidden=math.inf, prior_sigma_out=math.inf)  # d = 256


def test_unpack_and_predict(nf):
    g, X, w, ys = _data(4)
    tgt = nf.BNNTarget("normal", _t(X), HID)
    f = _network(X, ys)
    W, v, c = tgt.unpack(_t(ys[:, 0]))
    assert W.shape == (PF, HID) and v.shape == (HID,) and c.shape == ()
    for k in range(HID):
        assert np.array_equal(W[:, k].numpy(), ys[k * PF:(k + 1) * PF, 0])
    assert np.array_equal(v.numpy(), ys[HID * PF:HID * PF + HID, 0]) and float(c) == ys[-1, 0]
    Wb, vb, cb = tgt.unpack(_t(ys))
    assert Wb.shape == (PF, HID, NB) and vb.shape == (HID, NB) and cb.shape == (NB,)
    assert torch.equal(Wb[:, :, 2], tgt.unpack(_t(ys[:, 2]))[0])
    assert np.allclose(tgt.predict(_t(ys[:, 0]), _t(X)).numpy(), f[:, 0], rtol=0, atol=1e-14)
    assert np.allclose(tgt.predict(_t(ys), _t(X)).numpy(), f, rtol=0, atol=1e-14)
    Xn = g.standard_normal((4, PF))
    assert np.allclose(tgt.predict(_t(ys), _t(Xn)).numpy(), _network(Xn, ys), rtol=0, atol=1e-14)
    for bad in (lambda: tgt.unpack(_t(ys[:-1])), lambda: tgt.predict(_t(ys), _t(X[:, :1])), lambda: tgt.predict(_t(ys), _t(X[0]))):
        with pytest.raises(nf.NFHipError):
            bad()


def test_check_compatible_and_builtin_routing(nf):
    from normalizingflows_jl_amd import objectives as ob
    from normalizingflows_jl_amd.flows import check_target

    X = torch.randn(4, 2, generator=torch.Generator().manual_seed(0))
    tb = nf.BNNTarget("poisson", X, 2)
    tr = nf.BNNRegressionTarget(X, torch.tensor([0.5, -1.0, 0.0, 2.0]), 2)
    tc = nf.BNNClassifierTarget(X, torch.tensor([0, 1, 1, 0]), 2, link="probit")
    for t in (tb, tr, tc):
        assert t.d == 7 and isinstance(t, nf.BNNTarget) and isinstance(t, ob._BUILTIN) and isinstance(t, ob._LINPRED)
        check_target(t, torch.float32, "cpu", 7)
        for args in ((torch.float64, "cpu", 7), (torch.float32, "cuda:0", 7), (torch.float32, "cpu", 6)):
            with pytest.raises(nf.NFHipError):
                check_target(t, *args)

    class F:  # what _builtin reads of a flow
        def __init__(self, kind, d, inner=None):
            self.kind, self.theta, self.inner = kind, torch.zeros(1), inner
            self.dist = type("D", (), {"d": d})()

    for t in (tb, tr, tc):
        for kind in ("planar", "radial", "meanfield"):
            assert ob._builtin(F(kind, 7), t) is False   # the closure route, with the device score
        assert ob._builtin(F("hamiltonian", 14), t) is False
        for kind in ("realnvp", "nsf", "composite", "fullrank"):
            assert ob._builtin(F(kind, 7), t) is True    # the library route
        assert ob._builtin(F("preconditioned", 7, F("realnvp", 7)), t) is True
        with pytest.raises(nf.NFHipError):
            ob._builtin(F("planar", 6), t)
    wide = nf.BNNTarget("normal", torch.ones(4, 14), 16)  # d = 241: the library route
    for kind in ("realnvp", "nsf", "fullrank"):
        assert ob._builtin(F(kind, 241), wide) is True


# ---- the numpy form -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", bf.FAMILIES)
def test_the_form_is_the_derivative_of_its_value(family):
    """central differences in float64 at (3, 5, 33), every coordinate of W, v and c: the value's differences agree with the score to
    3e-7 of max(1, |score|) (measured when written: at most 3e-8)"""
    H, p, rows = 3, 5, 33
    X, scl, off, wt, par = bf.arrays(family, H, p, rows)
    p0 = bf.p0_of(scl, off, wt, par, H, p)
    d = bf.dim(H, p)
    y0 = bf.sample_ys(d, 1)
    sc = bf.logp_score(y0, X, p0, H, family)[1][:, 0]
    worst = 0.0
    for i in range(d):
        e = np.zeros_like(y0)
        e[i] = 1e-5
        fd = (bf.logp_score(y0 + e, X, p0, H, family)[0][0] - bf.logp_score(y0 - e, X, p0, H, family)[0][0]) / 2e-5
        worst = max(worst, abs(fd - sc[i]) / max(1.0, abs(sc[i])))
    print(f"bnn central differences {family}: {worst:.2e}")
    assert worst <= 3e-7, (family, worst)


def test_a_zero_weight_row_of_huge_features_leaves_the_form_alone():
    H, p, rows = 3, 5, 33
    X, scl, off, wt, par = bf.arrays("poisson", H, p, rows)
    ys = bf.sample_ys(bf.dim(H, p), 5)
    want = bf.logp_score(ys, X, bf.p0_of(scl, off, wt, par, H, p), H, "poisson")
    got = bf.logp_score(ys, np.vstack([X, np.full((1, p), 1e30)]), bf.p0_of(np.append(scl, 1.0), np.append(off, 0.0), np.append(wt, 0.0), par, H, p),
                        H, "poisson")
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


# ---- the float32 floor of the GPU tests' inputs -------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["logit", "normal", "student", "poisson"])
@pytest.mark.parametrize("shape", bf.SHAPES, ids=lambda s: "H%d_p%d_r%d" % s)
def test_the_float32_form_alone_stays_inside_the_tolerances(nf, shape, family):
    """the float32 form against the float64 one on the GPU tests' inputs, read back from the Float32 target the constructor folds
    (what the device reads), with y as drawn and scaled by 6: at most 0.3x the element-wise tolerance on log p and 0.2x GRAD_RTOL
    on the score (2e-5 of |g|inf), so the plain tolerances are expected to hold outright"""
    H, p, rows = shape
    d = bf.dim(H, p)
    X, scl, off, wt, par = bf.arrays(family, H, p, rows)
    assert (X[:, 0] == 1.0).all() and set(np.unique(wt)) <= set(bf.WEIGHTS)
    tgt = nf.BNNTarget(family, _t(X).float(), H, scale=_t(scl).float(), offset=_t(off).float(), weights=_t(wt).float(),
                       param=par if family == "student" else None, prior_sigma_hidden=bf.SIGMA_HIDDEN, prior_sigma_out=bf.SIGMA_OUT)
    Xd, p0 = bf.target_arrays(tgt)
    assert np.array_equal(Xd, X) and np.array_equal(p0[:3 * rows], np.concatenate([scl, off, wt]))
    assert np.allclose(p0, bf.p0_of(scl, off, wt, par, H, p), rtol=1e-7, atol=0)
    for scale in (1.0, 6.0):
        ys = bf.sample_ys(d, bf.N_FULL, scale=scale)
        l64, s64 = bf.logp_score(ys, Xd, p0, H, family)
        l32, s32 = bf.logp_score(ys.astype(np.float32), Xd, p0, H, family)
        assert l32.dtype == s32.dtype == np.float32 and np.isfinite(l64).all() and np.isfinite(s64).all()
        lr = float((np.abs(l32 - l64) / (P.Y_ATOL + P.Y_RTOL * np.abs(l64))).max())
        gr = float(np.abs(s32 - s64).max() / np.abs(s64).max()) / P.GRAD_RTOL
        print(f"bnn floor {family} {shape} y x{scale:g}: logp {lr:.4f}x, score {gr:.5f}x")
        assert lr <= 0.3 and gr <= 0.2, (shape, family, scale, lr, gr)


# ---- the float64 loop train_flow is compared with ------------------------------------------------------------------------------------
def fullrank_numpy_losses(X, p0, H, family, n, seed, lr, iters):
    """Full-rank Gaussian VI on the network posterior as a float64 numpy loop from theta = [0 ; I] (tests/fullrank_ref.py's layout):
    draws of stream i, the form's score, oracle Adam.  Returns the losses and theta."""
    import fullrank_ref as fr
    import nf_oracle as o

    d = bf.dim(H, X.shape[1])
    th = fr.join(np.zeros(d), np.eye(d))
    m, v = np.zeros_like(th), np.zeros_like(th)
    losses = []
    for i in range(iters):
        xs = o.base_sample(d, n, seed, 0, i, precision="f64")
        loss, g = fr.neg_elbo_value_and_grad(th, xs, lambda y: bf.logp_score(y, X, p0, H, family))
        losses.append(float(loss))
        o.adam_update(th, g, m, v, i + 1, lr=lr)  # in place
    return losses, th


TRAIN = ("normal", (2, 2, 33), 64, 9, 0.05, 6)  # family, shape, draws, seed, Adam's rate, steps


def train_target(nf, device="cpu"):
    family, (H, p, rows) = TRAIN[:2]
    X, scl, off, wt, par = bf.arrays(family, H, p, rows)
    to = lambda a: torch.tensor(a, dtype=torch.float64, device=device)
    return nf.BNNTarget(family, to(X), H, scale=to(scl), offset=to(off), weights=to(wt), prior_sigma_hidden=bf.SIGMA_HIDDEN,
                        prior_sigma_out=bf.SIGMA_OUT)


def test_the_numpy_training_loop_descends(nf):
    """the float64 loop alone descends, so the GPU comparison does not rest on luck"""
    family, (H, p, rows), n, seed, lr, iters = TRAIN
    tgt = train_target(nf)
    Xd, p0 = bf.target_arrays(tgt)
    losses, th = fullrank_numpy_losses(Xd, p0, H, family, n, seed, lr, iters)
    print("bnn fullrank numpy loop", losses)
    assert all(np.isfinite(losses)) and losses[-1] < losses[0] and np.isfinite(th).all()


# ---- resources ---------------------------------------------------------------------------------------------------------------------
def test_bnn_kernels_use_no_scratch_and_fit_their_launch_bounds(nf):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources

    rows = kernel_resources.kernel_table(os.path.join(ROOT, "normalizingflows.jl_amd", "build"))
    assert len(rows) > 200, "the objects' metadata notes were not readable"
    for prefix, count in (("void k_target_bnn_tiled<", 20), ("void k_target_bnn<", 10)):  # DB in {1, 2, 4, 8} x 5 phi; {float, double} x 5 phi
        hit = [r for r in rows if r[0].startswith(prefix)]
        assert len(hit) == count, (prefix, [r[0][:60] for r in hit])
        for name, agpr, vgpr, sgpr, scratch, lds in hit:
            assert scratch == 0, (name, scratch)
            assert vgpr <= 512, (name, vgpr)  # 256 threads per workgroup: one wave per SIMD may use the whole register file
            assert lds <= 4096, (name, lds)   # static LDS only (the tile and the images are dynamic)
            if re.search(r", [12]>\(", name[:80]):
                assert vgpr <= 256, (name, vgpr)  # DB <= 2: two workgroups per CU
