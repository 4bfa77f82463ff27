"""CPU checks of the softmax regression target (NF_TARGET_SOFTMAX, kind 15): the constant, nf_target_check's argument
conventions as nf_target_logp reports them BEFORE any device work (a stand-in context is enough), the refusals of the flows
that evaluate their target in their own kernels, the constructors' refusals, the host folding of SoftmaxRegressionTarget and
MultinomialRegressionTarget against the model written directly with scipy, the routing of the Python mirror, the float32
floor of the GPU tests' inputs, the float64 training loop test_gpu_softmax.py compares train_flow with, and the new kernels'
resources."""
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

import parity as P
import softmax_forms as sf
from __graft_entry__ import ROOT, build, load_package


@pytest.fixture(scope="module")
def nf():
    build()  # no-op when libnfhip.so is up to date
    return load_package()


def _standin():
    return C.cast((C.c_char * 4096)(), C.c_void_p)


def _t(a):
    return torch.tensor(np.asarray(a), dtype=torch.float64)


def test_constant_matches_the_header_and_kinds_7_and_14_stay_absent(nf):
    hdr = open(os.path.join(ROOT, "include", "nfhip.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"^#define (NF_TARGET_\w+) (\d+)", hdr, re.M)}
    assert defs["NF_TARGET_SOFTMAX"] == nf._lib.NF_TARGET_SOFTMAX == 15
    for name, v in defs.items():
        assert getattr(nf._lib, name) == v
    mirror = [v for k, v in vars(nf._lib).items() if k.startswith("NF_TARGET_")]
    for absent in (7, 14):
        assert absent not in defs.values() and absent not in mirror
    assert nf.load_library().nf_abi_version() == 4


def test_target_check_errors_come_before_device_work(nf):
    """NF_ERR_ARG (-1) for every violated convention of kind 15 without touching the context (N = 0: nothing is launched, and a
    good target's answer is no error).  d > 256 is answered by the launcher, as for the siblings: test_gpu_softmax.py."""
    from normalizingflows_jl_amd._lib import Target

    lib = nf.load_library()
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p).value
    ctx = _standin()

    def logp(t, d=6, n=4, dtype=0):
        return lib.nf_target_logp(ctx, dtype, C.byref(t), d, n, C.c_void_p(p), C.c_void_p(p), None)

    for dtype in (0, 1):
        assert logp(Target(15, 0, p, 8.0, 3.0), dtype=dtype) == -1             # p0 = NULL
        assert logp(Target(15, p, 0, 8.0, 3.0), dtype=dtype) == -1             # p1 = NULL
        assert logp(Target(15, p, p, 0.0, 3.0), dtype=dtype) == -1             # rows = 0
        assert logp(Target(15, p, p, -3.0, 3.0), dtype=dtype) == -1            # negative rows
        assert logp(Target(15, p, p, 2.5, 3.0), dtype=dtype) == -1             # rows not integral
        assert logp(Target(15, p, p, 2147483648.0, 3.0), dtype=dtype) == -1    # rows = 2^31
        assert logp(Target(15, p, p, math.nan, 3.0), dtype=dtype) == -1        # NaN rows
        assert logp(Target(15, p, p, 8.0, 1.0), dtype=dtype) == -1             # C = 1
        assert logp(Target(15, p, p, 8.0, 0.0), dtype=dtype) == -1             # C = 0
        assert logp(Target(15, p, p, 8.0, -2.0), dtype=dtype) == -1            # negative C
        assert logp(Target(15, p, p, 8.0, 17.0), d=34, dtype=dtype) == -1      # C = 17
        assert logp(Target(15, p, p, 8.0, 2.5), dtype=dtype) == -1             # C not integral
        assert logp(Target(15, p, p, 8.0, math.nan), dtype=dtype) == -1        # NaN C
        assert logp(Target(15, p, p, 8.0, math.inf), dtype=dtype) == -1
        assert logp(Target(15, p, p, 8.0, 4.0), dtype=dtype) == -1             # d % C != 0 (6 % 4)
        assert logp(Target(15, p, p, 8.0, 3.0), d=7, dtype=dtype) == -1        # d % C != 0 (7 % 3)
        assert logp(Target(15, p, p, 8.0, 3.0), n=0, dtype=dtype) >= 0         # past the check
        assert logp(Target(15, p, p, 8.0, 2.0), n=0, dtype=dtype) >= 0
        assert logp(Target(15, p, p, 8.0, 16.0), d=32, n=0, dtype=dtype) >= 0  # C at its cap
    assert logp(Target(7, p, p, 8.0, 2.0)) == -1 and logp(Target(14, p, p, 8.0, 2.0)) == -1  # no such kinds


def test_flows_that_evaluate_the_target_in_their_own_kernels_refuse_before_device_work(nf):
    """planar, radial, mean-field and Hamiltonian descriptors answer NF_ERR_UNSUPPORTED (-2) at all five ELBO entry points, with
    kind 15 as the target and as the Hamiltonian score -- the stand-in context is never used."""
    from normalizingflows_jl_amd._lib import NF_KIND, FlowDesc, Target

    lib = nf.load_library()
    buf = (C.c_double * 256)()
    p = C.cast(buf, C.c_void_p)
    ctx = _standin()
    val = C.c_double(0.0)

    def five(desc, tgt):
        return [lib.nf_elbo_value_and_grad(ctx, C.byref(desc), C.byref(tgt), p, p, 8, 8, 1, 0, 0, p),
                lib.nf_elbo_batch(ctx, C.byref(desc), C.byref(tgt), p, p, 8, None, C.byref(val)),
                lib.nf_elbo_batch_rng(ctx, C.byref(desc), C.byref(tgt), p, 8, 1, 0, 0, C.byref(val)),
                lib.nf_elbo_step(ctx, C.byref(desc), C.byref(tgt), p, p, p, 8, 1, 0, 1e-3, 0.9, 0.999, 1e-8, None, None),
                lib.nf_elbo_step_enqueue(ctx, C.byref(desc), C.byref(tgt), p, p, p, 8, 1, p, 1e-3, 0.9, 0.999, 1e-8, None)]

    diag = Target(0, p.value, p.value, 0.0, 0.0)
    smx = Target(15, p.value, p.value, 4.0, 2.0)
    for kind, dtype in (("planar", 0), ("radial", 0), ("meanfield", 1), ("planar", 1)):
        desc = FlowDesc()
        desc.kind, desc.dtype, desc.d, desc.nlayers = NF_KIND[kind], dtype, 4, 2
        assert five(desc, smx) == [-2] * 5, kind
    hd = FlowDesc()
    hd.kind, hd.dtype, hd.d, hd.nlayers, hd.K = NF_KIND["hamiltonian"], 0, 8, 2, 3
    hd.score = C.cast(C.pointer(diag), C.c_void_p)  # a supported score, a softmax ELBO target
    assert five(hd, smx) == [-2] * 5
    hd.score = C.cast(C.pointer(smx), C.c_void_p)   # a softmax score
    assert five(hd, diag) == [-2] * 5


# ---- host folding ---------------------------------------------------------------------------------------------------------------
CLS, PF, ROWS = 3, 2, 7


def _data(seed=0):
    g = np.random.default_rng(seed)
    X = g.standard_normal((ROWS, PF)) / np.sqrt(PF)
    X[:, 0] = 1.0
    w = g.uniform(0.3, 2.5, ROWS)
    w[2] = 0.0  # one dropped row
    ys = g.standard_normal((CLS * PF, 5))
    return g, X, w, ys


def _prior(ys, sigma):
    return stats.norm.logpdf(ys, 0.0, sigma).sum(0)


def _folded(tgt, ys):
    return sf.ref_of(tgt)(ys)[0]


def test_softmax_folding_against_log_softmax_and_a_normal_prior(nf):
    g, X, w, ys = _data(1)
    lab = g.integers(0, CLS, ROWS)
    tgt = nf.SoftmaxRegressionTarget(_t(X), torch.tensor(lab), CLS, weights=_t(w), prior_sigma=1.7, const=0.25)
    W = ys.reshape(CLS, PF, 5)                               # class-major
    logits = np.einsum("if,cfn->inc", X, W)                  # [rows, N, C]
    ll = sp.log_softmax(logits, axis=2)[np.arange(ROWS), :, lab]
    direct = 0.25 + (w[:, None] * ll).sum(0) + _prior(ys, 1.7)
    got = _folded(tgt, ys)
    assert got.shape == direct.shape == (5,)
    assert (np.abs(got - direct) <= 1e-12 * np.abs(direct)).all(), (got, direct)
    assert tgt.d == CLS * PF and tgt.p == PF and tgt.n_classes == CLS and tgt.rows == ROWS
    assert tgt.A.dtype == torch.float64 and tgt.p0.dtype == torch.float64 and tgt.p0.shape == (2 * ROWS + 2,)
    assert tgt.c.kind == 15 and tgt.c.p0 == tgt.p0.data_ptr() and tgt.c.p1 == tgt.A.data_ptr() and tgt.c.s0 == ROWS and tgt.c.s1 == CLS
    assert float(tgt.p0[-2]) == 1.0 / 1.7**2
    # the weights helper: W [p, C], logits = X W
    Wm = tgt.weights(_t(ys[:, 0]))
    assert Wm.shape == (PF, CLS) and np.allclose((_t(X) @ Wm).numpy(), logits[:, 0, :], rtol=0, atol=1e-14)
    assert tgt.weights(_t(ys)).shape == (PF, CLS, 5)
    # the score is the derivative of the value (central differences in float64)
    y0 = ys[:, :1]
    sc = sf.ref_of(tgt)(y0)[1][:, 0]
    for i in range(CLS * PF):
        e = np.zeros_like(y0)
        e[i] = 1e-6
        fd = (_folded(tgt, y0 + e)[0] - _folded(tgt, y0 - e)[0]) / 2e-6
        assert abs(fd - sc[i]) <= 1e-7 * max(1.0, abs(sc[i])), (i, fd, sc[i])
    # labels given as floats, classes inferred, defaults, the flat prior, Float32
    same = nf.SoftmaxRegressionTarget(_t(X), _t(lab.astype(np.float64)), CLS, weights=_t(w), prior_sigma=1.7, const=0.25)
    assert torch.equal(same.p0, tgt.p0)
    lab2 = np.array([0, 1, 2, 0, 1, 2, 0])
    inferred = nf.SoftmaxRegressionTarget(_t(X), torch.tensor(lab2))
    assert inferred.n_classes == 3 and torch.equal(inferred.p0[ROWS:2 * ROWS], torch.ones(ROWS).double())
    flat = nf.SoftmaxRegressionTarget(_t(X), torch.tensor(lab), CLS, weights=_t(w), prior_sigma=math.inf)
    assert float(flat.p0[-2]) == 0.0 and float(flat.p0[-1]) == 0.0
    assert (np.abs(_folded(flat, ys) - (w[:, None] * ll).sum(0)) <= 1e-12 * np.abs(direct)).all()
    t32 = nf.SoftmaxRegressionTarget(_t(X).float(), torch.tensor(lab), CLS)
    assert t32.A.dtype == torch.float32 and t32.p0.dtype == torch.float32


def test_multinomial_folding_against_scipy(nf):
    g, X, w, ys = _data(2)
    counts = g.integers(0, 4, (ROWS, CLS))
    counts[1] = 0        # a row without trials contributes log 1 = 0
    counts[4, 1] = 0
    tgt = nf.MultinomialRegressionTarget(_t(X), torch.tensor(counts), weights=_t(w), prior_sigma=2.0)
    W = ys.reshape(CLS, PF, 5)
    probs = sp.softmax(np.einsum("if,cfn->inc", X, W), axis=2)  # [rows, N, C]
    direct = sum(w[i] * stats.multinomial.logpmf(counts[i], counts[i].sum(), probs[i]) for i in range(ROWS)) + _prior(ys, 2.0)
    got = _folded(tgt, ys)
    assert (np.abs(got - direct) <= 1e-12 * np.abs(direct)).all(), (got, direct)
    assert tgt.rows == int((counts != 0).sum()) and tgt.d == CLS * PF and tgt.n_classes == CLS and tgt.c.kind == 15
    assert isinstance(tgt, nf.SoftmaxRegressionTarget)
    same = nf.MultinomialRegressionTarget(_t(X), _t(counts.astype(np.float64)), weights=_t(w), prior_sigma=2.0)
    assert torch.equal(same.p0, tgt.p0) and torch.equal(same.A, tgt.A)


def test_constructors_refuse_bad_arguments(nf):
    E = nf.NFHipError
    g, X, w, _ = _data(3)
    X, w = _t(X), _t(w)
    lab = torch.tensor([0, 1, 2, 0, 1, 2, 1])
    counts = torch.tensor(g.integers(0, 4, (ROWS, CLS)))
    bad = [
        lambda: nf.SoftmaxRegressionTarget(X[0], lab),                               # not a matrix
        lambda: nf.SoftmaxRegressionTarget(X.to(torch.float16), lab),
        lambda: nf.SoftmaxRegressionTarget(X * math.inf, lab),
        lambda: nf.SoftmaxRegressionTarget(X, lab[:-1]),                             # one label per row
        lambda: nf.SoftmaxRegressionTarget(X, lab.double() + 0.5),                   # not integral
        lambda: nf.SoftmaxRegressionTarget(X, -lab),                                 # negative
        lambda: nf.SoftmaxRegressionTarget(X, lab, 2),                               # a label out of range
        lambda: nf.SoftmaxRegressionTarget(X, lab.float()),                          # element types differ
        lambda: nf.SoftmaxRegressionTarget(X, lab * 0),                              # one class inferred
        lambda: nf.SoftmaxRegressionTarget(X, lab, 1),
        lambda: nf.SoftmaxRegressionTarget(X, lab, 17),
        lambda: nf.SoftmaxRegressionTarget(X, lab, 3.5),
        lambda: nf.SoftmaxRegressionTarget(torch.ones(4, 129, dtype=torch.float64), torch.tensor([0, 1, 0, 1])),  # C p = 258
        lambda: nf.SoftmaxRegressionTarget(torch.ones(4, 17, dtype=torch.float64), torch.tensor([0, 1, 0, 1]), 16),
        lambda: nf.SoftmaxRegressionTarget(X, lab, weights=-w),
        lambda: nf.SoftmaxRegressionTarget(X, lab, weights=w[:-1]),
        lambda: nf.SoftmaxRegressionTarget(X, lab, weights=w * math.nan),
        lambda: nf.SoftmaxRegressionTarget(X, lab, weights=w.to("meta")),            # devices differ
        lambda: nf.SoftmaxRegressionTarget(X, lab, prior_sigma=0.0),
        lambda: nf.SoftmaxRegressionTarget(X, lab, prior_sigma=-math.inf),
        lambda: nf.SoftmaxRegressionTarget(X, lab, prior_sigma=math.nan),
        lambda: nf.SoftmaxRegressionTarget(X, lab, const=math.nan),
        lambda: nf.SoftmaxRegressionTarget(X, lab, const=math.inf),
        lambda: nf.MultinomialRegressionTarget(X, counts[:-1]),                      # one row of counts per row of X
        lambda: nf.MultinomialRegressionTarget(X, counts[:, 0]),                     # not a matrix
        lambda: nf.MultinomialRegressionTarget(X, counts[:, :1]),                    # one class
        lambda: nf.MultinomialRegressionTarget(X, torch.ones(ROWS, 17, dtype=torch.int64)),
        lambda: nf.MultinomialRegressionTarget(X, -counts),
        lambda: nf.MultinomialRegressionTarget(X, counts.double() + 0.5),
        lambda: nf.MultinomialRegressionTarget(X, counts.float()),                   # element types differ
        lambda: nf.MultinomialRegressionTarget(X, counts * 0),                       # no observation at all
        lambda: nf.MultinomialRegressionTarget(X, counts, weights=-w),
        lambda: nf.MultinomialRegressionTarget(X, counts, prior_sigma=0.0),
    ]
    for i, make in enumerate(bad):
        with pytest.raises(E):
            make()
            pytest.fail(f"case {i} was accepted")
    nf.SoftmaxRegressionTarget(X, lab, 16, weights=w, prior_sigma=math.inf)  # unused classes, zero weights, a flat prior: fine
    nf.SoftmaxRegressionTarget(torch.ones(4, 128, dtype=torch.float64), torch.tensor([0, 1, 0, 1]))  # C p = 256


def test_check_compatible_and_builtin_routing(nf):
    from normalizingflows_jl_amd import objectives as ob
    from normalizingflows_jl_amd.flows import check_target

    X = torch.randn(4, 2, generator=torch.Generator().manual_seed(0))
    ts = nf.SoftmaxRegressionTarget(X, torch.tensor([0, 2, 1, 1]))
    tm = nf.MultinomialRegressionTarget(X, torch.tensor([[1, 0, 2], [0, 0, 1], [3, 1, 0], [0, 2, 2]]))
    for t in (ts, tm):
        assert t.d == 6 and isinstance(t, ob._BUILTIN) and isinstance(t, ob._LINPRED)
        check_target(t, torch.float32, "cpu", 6)
        for args in ((torch.float64, "cpu", 6), (torch.float32, "cuda:0", 6), (torch.float32, "cpu", 4)):
            with pytest.raises(nf.NFHipError):
                check_target(t, *args)

    class F:  # what _builtin reads of a flow
        def __init__(self, kind, d):
            self.kind, self.theta = kind, torch.zeros(1)
            self.dist = type("D", (), {"d": d})()

    for t in (ts, tm):
        for kind in ("planar", "radial", "meanfield"):
            assert ob._builtin(F(kind, 6), t) is False   # the closure route, with the device score
        assert ob._builtin(F("hamiltonian", 12), t) is False
        for kind in ("realnvp", "nsf", "composite", "fullrank"):
            assert ob._builtin(F(kind, 6), t) is True    # the library route
        with pytest.raises(nf.NFHipError):
            ob._builtin(F("planar", 4), t)
    wide = nf.SoftmaxRegressionTarget(torch.ones(4, 25), torch.tensor([0, 9, 1, 1]))  # d = 250: the library route (no d = 64 stop as the mixture has)
    for kind in ("realnvp", "nsf", "fullrank"):
        assert ob._builtin(F(kind, 250), wide) is True


# ---- the float32 floor of the GPU tests' inputs -------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sf.SHAPES + [(10, 25, 200)], ids=lambda s: "C%d_p%d_r%d" % s)
def test_the_float32_form_alone_stays_far_inside_the_tolerances(nf, shape):
    """the float32 form against the float64 one on the GPU tests' inputs, read back from the Float32 target the constructor folds
    (what the device reads): at most 0.25x the element-wise tolerance on log p and 0.05x GRAD_RTOL on the score, so the `floor=`
    clause never decides a nf_target_logp check (measured when written: at most 0.027x and 0.003x)"""
    C_, p, rows = shape
    d = C_ * p
    X, lab, wt = sf.arrays(C_, p, rows)
    assert (X[:, 0] == 1.0).all() and set(np.unique(wt)) <= set(sf.WEIGHTS)
    tgt = nf.SoftmaxRegressionTarget(_t(X).float(), _t(lab).float(), C_, weights=_t(wt).float(), prior_sigma=sf.SIGMA)
    Xd, p0 = sf.target_arrays(tgt)
    assert np.array_equal(Xd, X) and np.array_equal(p0[:2 * rows], np.concatenate([lab, wt]))
    assert np.allclose(p0, sf.p0_of(lab, wt, d), rtol=1e-7, atol=0)
    for n in (sf.n_of(shape) if shape in sf.SHAPES else (sf.N_FULL,)):
        ys = sf.sample_ys(d, n)
        l64, s64 = sf.logp_score(ys, Xd, p0, C_)
        l32, s32 = sf.logp_score(ys.astype(np.float32), Xd, p0, C_)
        assert l32.dtype == s32.dtype == np.float32
        lr = float((np.abs(l32 - l64) / (P.Y_ATOL + P.Y_RTOL * np.abs(l64))).max())
        gr = float(np.abs(s32 - s64).max() / np.abs(s64).max()) / P.GRAD_RTOL
        print(f"softmax floor {shape} N={n}: logp {lr:.4f}x, score {gr:.5f}x")
        assert lr <= 0.25 and gr <= 0.05, (shape, n, lr, gr)


# ---- the float64 loop train_flow is compared with ------------------------------------------------------------------------------------
def fullrank_numpy_losses(X, p0, C_, n, seed, lr, iters):
    """Full-rank Gaussian VI on the softmax posterior as a float64 numpy loop from theta = [0 ; I] (tests/fullrank_ref.py's
    layout): draws of stream i, the form's score, oracle Adam on the shift and the lower triangle (the strict upper triangle has
    a zero gradient and stays 0).  Returns the losses and theta."""
    import fullrank_ref as fr
    import nf_oracle as o

    d = C_ * X.shape[1]
    th = fr.join(np.zeros(d), np.eye(d))
    m, v = np.zeros_like(th), np.zeros_like(th)
    losses = []
    for i in range(iters):
        xs = o.base_sample(d, n, seed, 0, i, precision="f64")
        loss, g = fr.neg_elbo_value_and_grad(th, xs, lambda y: sf.logp_score(y, X, p0, C_))
        losses.append(float(loss))
        o.adam_update(th, g, m, v, i + 1, lr=lr)  # in place
    return losses, th


def test_the_numpy_training_loop_descends(nf):
    """(3, 2, 33), seed 9, Adam(0.05), 64 draws, six steps on the Float64 target's own buffers: the float64 loop alone descends, so
    the GPU comparison does not rest on luck"""
    X, lab, wt = sf.arrays(3, 2, 33)
    tgt = nf.SoftmaxRegressionTarget(_t(X), _t(lab), 3, weights=_t(wt), prior_sigma=sf.SIGMA)
    Xd, p0 = sf.target_arrays(tgt)
    assert np.allclose(p0, sf.p0_of(lab, wt, 6), rtol=1e-15, atol=0)
    losses, th = fullrank_numpy_losses(Xd, p0, 3, 64, 9, 0.05, 6)
    print("softmax fullrank numpy loop", losses)
    assert all(np.isfinite(losses)) and losses[5] < losses[0] and np.isfinite(th).all()


# ---- resources ---------------------------------------------------------------------------------------------------------------------
def test_softmax_kernels_use_no_scratch_and_fit_their_launch_bounds(nf):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources

    rows = kernel_resources.kernel_table(os.path.join(ROOT, "normalizingflows.jl_amd", "build"))
    assert len(rows) > 200, "the objects' metadata notes were not readable"
    for prefix, count in (("void k_target_softmax_tiled<", 4), ("void k_target_softmax<", 2)):  # DB in {1, 2, 4, 8}; {float, double}
        hit = [r for r in rows if r[0].startswith(prefix)]
        assert len(hit) == count, (prefix, [r[0][:60] for r in hit])
        for name, agpr, vgpr, sgpr, scratch, lds in hit:
            assert scratch == 0, (name, scratch)
            assert vgpr <= 512, (name, vgpr)  # 256 threads per workgroup: one wave per SIMD may use the whole register file
            assert lds <= 4096, (name, lds)   # static LDS only (the tile and the images are dynamic)
