"""CPU checks of the Gaussian-mixture target (NF_TARGET_GAUSSMIX): the constant, the argument conventions of
nf_target_check as the C entry points report them BEFORE any device work (a stand-in context is enough), the refusals, the
host-side packing of MixtureTarget, the closed form this module and tests/test_gpu_mixture.py share (checked against the
oracle's Cross density), and the scratch of the tiled kernel.

The closed form is dtype-generic (float32 arrays are evaluated in float32) and is written on the PACKED parameters the device
reads -- the stacked W_k = inv(L_k), the common centre mbar, b_k = W_k (mu_k - mbar) and c_k -- so that a Float32 reference
sees the same rounded numbers as the kernel; pack_mixture is the float64 numpy packing from (pi, mu, Sigma)."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

from __graft_entry__ import ROOT, build, load_package

L2PI = float(np.log(2.0 * np.pi))


# ---- the closed form ---------------------------------------------------------------------------------------------------------
def pack_mixture(pi, mus, Sigmas):
    """float64: (pi (K,), mus (K, d), Sigmas (K, d, d)) -> (mbar (d,), b (K, d), c (K,), W (K, d, d)), zero weights dropped"""
    pi, mus, Sigmas = np.asarray(pi, np.float64), np.asarray(mus, np.float64), np.asarray(Sigmas, np.float64)
    pi = pi / pi.sum()
    keep = pi > 0
    pi, mus, Sigmas = pi[keep], mus[keep], Sigmas[keep]
    d = mus.shape[1]
    L = np.stack([np.linalg.cholesky(S) for S in Sigmas])
    W = np.stack([np.tril(np.linalg.solve(Lk, np.eye(d))) for Lk in L])
    mbar = (pi[:, None] * mus).sum(0)
    b = np.einsum("kij,kj->ki", W, mus - mbar[None, :])
    c = np.log(pi) - np.log(np.diagonal(L, axis1=1, axis2=2)).sum(1) - 0.5 * d * L2PI
    return mbar, b, c, W


def mixture_logp_score(y, mbar, b, c, W):
    """log p and its gradient at y (d, N), every array in y's element type:
    u_k = W_k (y - mbar) - b_k, q_k = c_k - |u_k|^2 / 2, log p = logsumexp_k q_k, grad = -sum_k r_k W_k' u_k"""
    t = y.dtype.type
    yc = y - mbar[:, None]
    u = np.einsum("kij,jn->kin", W, yc) - b[:, :, None]     # (K, d, N)
    q = c[:, None] - t(0.5) * (u * u).sum(1)                 # (K, N)
    m = q.max(0)
    e = np.exp(q - m[None, :])
    s = e.sum(0)
    r = e / s[None, :]
    g = -np.einsum("kif,kin->kfn", W, u)                     # (K, d, N): -W_k' u_k
    return m + np.log(s), (r[:, None, :] * g).sum(0)


def cast_pack(pack, dtype):
    return tuple(np.asarray(a, dtype=dtype) for a in pack)


def target_pack(tgt):
    """the packed parameters a MixtureTarget holds, as float64 numpy (exactly the values the device reads)"""
    d, K = tgt.d, tgt.K
    p0 = tgt.p0.double().cpu().numpy()
    return p0[:d], p0[d:d + K * d].reshape(K, d), p0[d + K * d:], tgt.A.double().cpu().numpy().reshape(K, d, d)


def cross_params(mu=2.0, sigma=0.15):
    """Cross(mu, sigma), example/targets/cross.jl:30-37: four equally weighted components; the vectors are standard deviations"""
    means = np.array([[0.0, mu], [-mu, 1.0], [mu, 1.0], [0.0, -mu]])
    stds = np.array([[sigma, 1.0], [1.0, sigma], [1.0, sigma], [sigma, 1.0]])
    return np.full(4, 0.25), means, np.stack([np.diag(s * s) for s in stds])


def random_mixture(d, K, seed=11):
    """Sigma_k = Q diag(lambda) Q', lambda in [0.5, 2]; means 3 randn(d) / sqrt(d); weights uniform in [0.5, 1.5], normalised"""
    rng = np.random.default_rng(seed + 100 * d + K)
    Sig = []
    for _ in range(K):
        Q, _ = np.linalg.qr(rng.standard_normal((d, d)))
        S = (Q * rng.uniform(0.5, 2.0, d)) @ Q.T
        Sig.append(0.5 * (S + S.T))
    mus = 3.0 * rng.standard_normal((K, d)) / np.sqrt(d)
    pi = rng.uniform(0.5, 1.5, K)
    return pi / pi.sum(), mus, np.stack(Sig)


# ---- tests -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nf():
    build()  # no-op when libnfhip.so is up to date
    return load_package()


def _standin():
    return C.cast((C.c_char * 4096)(), C.c_void_p)


def test_constant_matches_the_header(nf):
    hdr = open(os.path.join(ROOT, "include", "nfhip.h")).read()
    defs = dict(re.findall(r"^#define (NF_TARGET_\w+) (\d+)", hdr, re.M))
    assert int(defs["NF_TARGET_GAUSSMIX"]) == nf._lib.NF_TARGET_GAUSSMIX == 8
    assert "7" not in defs.values()  # kind 7 stays unassigned


def test_target_logp_argument_errors_come_before_device_work(nf):
    from normalizingflows_jl_amd._lib import Target

    lib = nf.load_library()
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p).value
    ctx = _standin()

    def logp(t, d=3, dtype=0):
        return lib.nf_target_logp(ctx, dtype, C.byref(t), d, 4, C.c_void_p(p), C.c_void_p(p), None)

    for dtype in (0, 1):
        assert logp(Target(8, 0, p, 2.0, 0.0), dtype=dtype) == -1              # p0 = NULL
        assert logp(Target(8, p, 0, 2.0, 0.0), dtype=dtype) == -1              # p1 = NULL
        assert logp(Target(8, p, p, 0.0, 0.0), dtype=dtype) == -1              # no component
        assert logp(Target(8, p, p, -2.0, 0.0), dtype=dtype) == -1
        assert logp(Target(8, p, p, 2.5, 0.0), dtype=dtype) == -1              # not integral
        assert logp(Target(8, p, p, 2147483648.0, 0.0), dtype=dtype) == -1     # too large
        assert logp(Target(8, p, p, 715827883.0, 0.0), dtype=dtype) == -1      # K d = 2^31 + 1 at d = 3
        assert logp(Target(8, p, p, float("nan"), 0.0), dtype=dtype) == -1
        assert logp(Target(8, p, p, 2.0, 1.0), dtype=dtype) == -1              # s1 must be 0


def test_flows_that_evaluate_the_target_in_their_own_kernels_refuse_before_device_work(nf):
    from normalizingflows_jl_amd._lib import NF_KIND, FlowDesc, Target

    lib = nf.load_library()
    buf = (C.c_double * 256)()
    p = C.cast(buf, C.c_void_p)
    ctx = _standin()
    val = C.c_double(0.0)
    tgt = Target(8, p.value, p.value, 4.0, 0.0)

    def all_entry_points(desc, target):
        return [lib.nf_elbo_value_and_grad(ctx, C.byref(desc), C.byref(target), p, p, 8, 8, 1, 0, 0, p),
                lib.nf_elbo_batch(ctx, C.byref(desc), C.byref(target), p, p, 8, None, C.byref(val)),
                lib.nf_elbo_batch_rng(ctx, C.byref(desc), C.byref(target), p, 8, 1, 0, 0, C.byref(val)),
                lib.nf_elbo_step(ctx, C.byref(desc), C.byref(target), p, p, p, 8, 1, 0, 1e-3, 0.9, 0.999, 1e-8, None, None),
                lib.nf_elbo_step_enqueue(ctx, C.byref(desc), C.byref(target), p, p, p, 8, 1, p, 1e-3, 0.9, 0.999, 1e-8, None)]

    for kind, dtype in (("planar", 0), ("radial", 0), ("meanfield", 1)):
        desc = FlowDesc()
        desc.kind, desc.dtype, desc.d, desc.nlayers = NF_KIND[kind], dtype, 3, 2
        assert all_entry_points(desc, tgt) == [-2] * 5, kind
    diag = Target(0, p.value, p.value, 0.0, 0.0)
    hd = FlowDesc()
    hd.kind, hd.dtype, hd.d, hd.nlayers, hd.K = NF_KIND["hamiltonian"], 0, 4, 2, 3
    hd.score = C.cast(C.pointer(tgt), C.c_void_p)       # the mixture as the integrator's score
    assert all_entry_points(hd, diag) == [-2] * 5
    hd.score = C.cast(C.pointer(diag), C.c_void_p)      # a supported score, the mixture as the ELBO target of the joint
    assert all_entry_points(hd, tgt) == [-2] * 5


def test_wide_float32_coupling_flows_refuse_before_device_work(nf):
    """The tiled kernel is built for d <= 64.  A Float32 RealNVP flow beyond it (d = 70, hidden (128, 100): a weight-streaming
    shape) answers NF_ERR_UNSUPPORTED at every ELBO entry point before the context is used."""
    from normalizingflows_jl_amd._lib import NF_KIND, FlowDesc, Target

    lib = nf.load_library()
    buf = (C.c_double * 256)()
    p = C.cast(buf, C.c_void_p)
    ctx = _standin()
    val = C.c_double(0.0)
    d = FlowDesc()
    d.kind, d.dtype, d.d, d.nlayers, d.n_hidden = NF_KIND["realnvp"], 0, 70, 2, 2
    d.hdims[0], d.hdims[1] = 128, 100
    tgt = Target(8, p.value, p.value, 2.0, 0.0)
    assert lib.nf_elbo_value_and_grad(ctx, C.byref(d), C.byref(tgt), p, p, 8, 8, 1, 0, 0, p) == -2
    assert lib.nf_elbo_batch(ctx, C.byref(d), C.byref(tgt), p, p, 8, None, C.byref(val)) == -2
    assert lib.nf_elbo_batch_rng(ctx, C.byref(d), C.byref(tgt), p, 8, 1, 0, 0, C.byref(val)) == -2
    assert lib.nf_elbo_step(ctx, C.byref(d), C.byref(tgt), p, p, p, 8, 1, 0, 1e-3, 0.9, 0.999, 1e-8, None, None) == -2
    assert lib.nf_elbo_step_enqueue(ctx, C.byref(d), C.byref(tgt), p, p, p, 8, 1, p, 1e-3, 0.9, 0.999, 1e-8, None) == -2


def test_packing_against_numpy(nf):
    pi, mus, Sig = random_mixture(7, 4)
    pi = np.concatenate([pi[:2] * 1.0, [0.0], pi[2:]])  # a zero-weight component in the middle: dropped
    pi = pi / pi.sum()
    mus = np.concatenate([mus[:2], 50.0 * np.ones((1, 7)), mus[2:]])
    Sig = np.concatenate([Sig[:2], np.eye(7)[None], Sig[2:]])
    t = nf.MixtureTarget(torch.tensor(pi), torch.tensor(mus), torch.tensor(Sig))
    assert (t.d, t.K) == (7, 4) and t.A.shape == (28, 7) and t.p0.shape == (7 + 28 + 4,) and t.A.dtype == torch.float64
    mbar, b, c, W = pack_mixture(pi, mus, Sig)
    gm, gb, gc, gW = target_pack(t)
    assert np.abs(gm - mbar).max() <= 1e-13 and np.abs(gb - b).max() <= 1e-12 and np.abs(gc - c).max() <= 1e-12
    assert np.abs(gW - W).max() <= 1e-12
    assert all(float(np.abs(np.triu(gW[k], 1)).max()) == 0.0 for k in range(4))  # lower triangular, stored dense with its zeros
    for k in range(4):
        Wi = np.linalg.inv(gW[k])
        assert np.abs(Wi @ Wi.T - np.delete(Sig, 2, axis=0)[k]).max() <= 1e-12
    assert t.c.kind == 8 and t.c.p0 == t.p0.data_ptr() and t.c.p1 == t.A.data_ptr() and t.c.s0 == 4.0 and t.c.s1 == 0.0
    # weights within 1e-6 of a unit sum are renormalised in float64
    t2 = nf.MixtureTarget(torch.tensor(pi * (1.0 + 5e-7)), torch.tensor(mus), torch.tensor(Sig))
    assert np.abs(target_pack(t2)[2] - c).max() <= 1e-12
    t32 = nf.MixtureTarget(torch.tensor(pi).float(), torch.tensor(mus).float(), torch.tensor(Sig).float())
    assert t32.A.dtype == torch.float32 and t32.p0.dtype == torch.float32 and t32.K == 4


def test_constructor_refuses_bad_arguments(nf):
    E = nf.NFHipError
    w = torch.tensor([0.5, 0.5], dtype=torch.float64)
    mu = torch.zeros(2, 3, dtype=torch.float64)
    S = torch.eye(3, dtype=torch.float64).repeat(2, 1, 1)
    nf.MixtureTarget(w, mu, S)
    with pytest.raises(E):
        nf.MixtureTarget(torch.tensor([0.5, 0.6], dtype=torch.float64), mu, S)      # does not sum to 1
    with pytest.raises(E):
        nf.MixtureTarget(torch.tensor([1.5, -0.5], dtype=torch.float64), mu, S)     # a negative weight
    with pytest.raises(E):
        nf.MixtureTarget(w.float(), mu, S)                                          # element types differ
    with pytest.raises(E):
        nf.MixtureTarget(w, mu, torch.eye(4, dtype=torch.float64).repeat(2, 1, 1))  # dimensions differ
    with pytest.raises(E):
        nf.MixtureTarget(torch.ones(1, dtype=torch.float64), mu, S)                 # one weight, two components
    bad = S.clone()
    bad[1] = torch.tensor([[1.0, 2.0, 0.0], [2.0, 1.0, 0.0], [0.0, 0.0, 1.0]], dtype=torch.float64)
    with pytest.raises(E, match="component 1.*positive definite"):
        nf.MixtureTarget(w, mu, bad)
    bad[1] = torch.tensor([[1.0, 0.5, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]], dtype=torch.float64)
    with pytest.raises(E, match="component 1.*symmetric"):
        nf.MixtureTarget(w, mu, bad)
    # a zero-weight component is dropped before it is factored: its Sigma is never looked at
    nf.MixtureTarget(torch.tensor([1.0, 0.0], dtype=torch.float64), mu, bad)


def test_check_compatible_and_routing(nf):
    from normalizingflows_jl_amd import objectives as ob
    from normalizingflows_jl_amd.flows import check_target

    E = nf.NFHipError
    t = nf.MixtureTarget(torch.tensor([0.25, 0.75]), torch.zeros(2, 3), torch.eye(3).repeat(2, 1, 1))
    check_target(t, torch.float32, "cpu", 3)
    t.check_compatible(torch.float32, "cpu", 3)
    for args in ((torch.float64, "cpu", 3), (torch.float32, "cuda:0", 3), (torch.float32, "cpu", 4)):
        with pytest.raises(E):
            check_target(t, *args)
    assert nf.MixtureTarget in ob._BUILTIN

    class F:  # what _builtin reads of a flow
        def __init__(self, kind, d, dtype=torch.float32):
            self.kind, self.theta = kind, torch.zeros(1, dtype=dtype)
            self.dist = type("D", (), {"d": d})()

    for kind in ("planar", "radial", "meanfield"):
        assert ob._builtin(F(kind, 3), t) is False
    assert ob._builtin(F("hamiltonian", 6), t) is False
    for kind in ("realnvp", "nsf", "composite"):
        assert ob._builtin(F(kind, 3), t) is True
    wide = nf.MixtureTarget(torch.ones(1), torch.zeros(1, 70), torch.eye(70)[None])
    assert ob._builtin(F("realnvp", 70), wide) is False  # the library refuses it: the closure route
    wide64 = nf.MixtureTarget(torch.ones(1, dtype=torch.float64), torch.zeros(1, 70, dtype=torch.float64), torch.eye(70, dtype=torch.float64)[None])
    assert ob._builtin(F("realnvp", 70, torch.float64), wide64) is True


def test_closed_form_at_the_cross_parameters_is_the_oracles_cross():
    import nf_oracle as o

    pack = pack_mixture(*cross_params(2.0, 0.15))
    y = 2.5 * np.random.default_rng(4).standard_normal((2, 50))
    lp, sc = mixture_logp_score(y, *pack)
    assert np.abs(lp - o.cross_logp(y, 2.0, 0.15)).max() <= 1e-11
    assert np.abs(sc - o.cross_grad(y, 2.0, 0.15)).max() <= 1e-11 * max(1.0, np.abs(sc).max())
    l32, s32 = mixture_logp_score(y.astype(np.float32), *cast_pack(pack, np.float32))
    assert l32.dtype == np.float32 and s32.dtype == np.float32  # dtype-generic: float32 in, float32 arithmetic


def test_tiled_mixture_kernels_use_no_scratch(nf):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources

    rows = [r for r in kernel_resources.kernel_table(os.path.join(ROOT, "normalizingflows.jl_amd", "build")) if "k_target_mixture" in r[0]]
    tiled = [r for r in rows if "k_target_mixture_tiled<" in r[0]]
    flat = [r for r in rows if "k_target_mixture<" in r[0]]
    assert len(tiled) == 2 and len(flat) == 2, [r[0][:60] for r in rows]  # DB in {1, 2}; {float, double}
    for name, agpr, vgpr, sgpr, scratch, lds in rows:
        assert scratch == 0, (name, scratch)
        assert vgpr <= 512, (name, vgpr)  # 256 threads per workgroup: one wave per SIMD may use the whole file
