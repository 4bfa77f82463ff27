"""Host-side mirror of the reference's flow constructors and of the Bijectors.jl surface the
hot path uses.  All arithmetic is done by libnfhip.so (HIP, gfx950); this module only owns
descriptors, the flat parameter vector and argument marshalling.

Reference files mirrored (paths in the reference checkout):
  src/flows/utils.jl            create_flow, fnn layout
  src/flows/planar_radial.jl    planarflow, radialflow
  src/flows/realnvp.jl          AffineCoupling, RealNVP_layer, realnvp
  src/flows/neuralspline.jl     NeuralSplineCoupling, NSF_layer, nsf
  src/NormalizingFlows.jl       _device_specific_rand (:94-127)

Array convention = the reference's: a batch is a (d, N) matrix with one sample per COLUMN,
stored column-major (here: a torch tensor of shape (d, N) whose transpose is contiguous).
A vector of shape (d,) is a single sample and gives scalar log-determinants
(src/flows/realnvp.jl:69-75).
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import Base, FlowDesc, NFHipError, Target, check, context_for


def _dtype_code(dt: torch.dtype) -> int:
    if dt == torch.float32:
        return _lib.NF_DTYPE_F32
    if dt == torch.float64:
        return _lib.NF_DTYPE_F64
    raise NFHipError(f"unsupported parameter type {dt}")


def new_batch(d: int, n: int, dtype, device) -> torch.Tensor:
    """(d, n) matrix in the reference's column-major layout."""
    return torch.empty((n, d), dtype=dtype, device=device).t()


def as_batch(x: torch.Tensor):
    """Returns (matrix (d, N) column-major, was_vector)."""
    vec = x.dim() == 1
    if vec:
        x = x.reshape(-1, 1)
    if x.dim() != 2:
        raise NFHipError("expected a vector (d,) or a matrix (d, N)")
    if not x.t().is_contiguous():
        x = x.t().contiguous().t()
    return x, vec


def _ptr(t: Optional[torch.Tensor]):
    return C.c_void_p(0 if t is None else t.data_ptr())


# --------------------------------------------------------------------------------------
# base distribution and RNG seam
# --------------------------------------------------------------------------------------
class MvNormal:
    """Distributions.MvNormal as the reference uses it for q0.

    MvNormal(d)            -> MvNormal(zeros(T, d), I): the base of every reference flow config (test/flow.jl:9,
                              example/demo_planar_flow.jl:24); the form the fused kernels draw in registers.
    MvNormal(mu, Sigma)    -> general base: Sigma a vector of VARIANCES (Diagonal(Sigma)) or a d x d covariance matrix
                              (Cholesky-factored here, once, on the host side of the boundary).  Draws are mu + L eps
                              (`unwhiten`, ext/NormalizingFlowsCUDAExt.jl:43-48; dense Sigma: test/ext/CUDA/cuda.jl:33-45).
    q0 is a leaf of destructure (@leaf MvNormal): none of this is trainable."""

    def __init__(self, mu_or_d, cov: Optional[torch.Tensor] = None):
        if cov is None and not torch.is_tensor(mu_or_d):
            self.d, self.mu, self.scale, self.c = int(mu_or_d), None, None, None
            return
        mu = mu_or_d
        if cov is None:
            raise NFHipError("MvNormal(mu, Sigma): give the covariance (a vector of variances or a matrix)")
        if mu.dim() != 1 or cov.shape[0] != mu.numel() or cov.dtype != mu.dtype or cov.device != mu.device:
            raise NFHipError("MvNormal(mu, Sigma): mu (d,), Sigma (d,) or (d, d), one element type and device")
        self.d = mu.numel()
        self.mu = mu.contiguous()
        if cov.dim() == 1:
            if not bool((cov > 0).all()):
                raise NFHipError("MvNormal: variances must be positive")
            self.scale = cov.sqrt().contiguous()
            kind, logdet = _lib.NF_BASE_DIAG, float(self.scale.double().log().sum())
        else:
            L = torch.linalg.cholesky(cov)  # raises for a matrix that is not positive definite, as PDMats does
            self.scale = L.t().contiguous()  # column-major lower triangle: element (i, k) at [k * d + i]
            kind, logdet = _lib.NF_BASE_DENSE, float(torch.diagonal(L).double().log().sum())
        self.c = Base(kind, self.mu.data_ptr(), self.scale.data_ptr(), logdet)

    @property
    def standard(self) -> bool:
        return self.c is None

    def base_ptr(self):
        return None if self.c is None else C.byref(self.c)

    def __len__(self):
        return self.d


class PhiloxRNG:
    """Device RNG handle (the analogue of CUDA.RNG in ext/NormalizingFlowsCUDAExt.jl).
    Philox4x32-10 keyed by `seed`; every draw call consumes one stream id, so successive
    calls give independent batches, and `sample_offset` places a shard inside a global batch."""

    def __init__(self, seed: int = 0, sample_offset: int = 0):
        self.seed = int(seed)
        self.stream = 0
        self.sample_offset = int(sample_offset)

    def next_stream(self) -> int:
        s = self.stream
        self.stream += 1
        return s


def device_specific_rand(rng: PhiloxRNG, dist, n: Optional[int] = None, *, device=None, dtype=torch.float32):
    """NormalizingFlows._device_specific_rand(rng, dist[, n])  (src/NormalizingFlows.jl:94-127).
    `dist` is an MvNormal base or a Flow (then base draws are pushed through the transform,
    as rand(td, n) does)."""
    if isinstance(dist, Flow):
        flow = dist
        nn = 1 if n is None else int(n)
        y = new_batch(flow.dist.d, nn, flow.theta.dtype, flow.theta.device)
        ctx = flow.ctx
        check(ctx.lib.nf_flow_rand(ctx.ptr, C.byref(flow.desc), _ptr(flow.theta), nn, rng.seed, rng.sample_offset,
                                   rng.next_stream(), _ptr(y)))
        return y[:, 0] if n is None else y
    if not dist.standard:
        device, dtype = dist.mu.device, dist.mu.dtype
    device = torch.device(device if device is not None else "cuda")
    nn = 1 if n is None else int(n)
    x = new_batch(dist.d, nn, dtype, device)
    ctx = context_for(device)
    check(ctx.lib.nf_base_rand(ctx.ptr, _dtype_code(dtype), dist.base_ptr(), dist.d, nn, rng.seed, rng.sample_offset,
                               rng.next_stream(), _ptr(x), _ptr(None)))
    return x[:, 0] if n is None else x


# --------------------------------------------------------------------------------------
# flows
# --------------------------------------------------------------------------------------
class Transform:
    """flow.transform: a composed bijector.  `inverse(t)` gives the Inverse{...} view."""

    def __init__(self, flow: "Flow", inverted: bool = False, layer: Optional[int] = None):
        self.flow = flow
        self.inverted = inverted
        self.layer = layer

    def __call__(self, x):
        return with_logabsdet_jacobian(self, x)[0]


class Flow:
    """Bijectors.TransformedDistribution: `dist` (base) + `transform`.  `theta` is the flat
    parameter vector of Optimisers.destructure(flow) (src/NormalizingFlows.jl:67)."""

    def __init__(self, kind: str, dist: MvNormal, nlayers: int, hdims: Sequence[int] = (), K: int = 0, B: float = 0.0,
                 dtype=torch.float32, device="cuda", theta: Optional[torch.Tensor] = None, score=None):
        self.kind, self.dist, self.nlayers = kind, dist, int(nlayers)
        self.score = score  # Hamiltonian flows: the target whose score drives LeapFrog (kept alive here)
        self.hdims, self.K, self.B = tuple(int(h) for h in hdims), int(K), float(B)
        if len(self.hdims) > _lib.NF_MAX_HIDDEN:
            raise NFHipError("at most 4 hidden layers")
        self.desc = FlowDesc()
        self.desc.kind = _lib.NF_KIND[kind]
        self.desc.dtype = _dtype_code(dtype)
        self.desc.d = dist.d
        self.desc.nlayers = self.nlayers
        self.desc.n_hidden = len(self.hdims)
        for i, h in enumerate(self.hdims):
            self.desc.hdims[i] = h
        self.desc.K = self.K
        self.desc.B = self.B
        self.desc.score = C.addressof(score.c) if score is not None else None
        if not dist.standard:
            if dist.mu.dtype != dtype:
                raise NFHipError(f"base distribution is {dist.mu.dtype}, flow parameters are {dtype}")
            self.desc.base = C.addressof(dist.c)  # kept alive by self.dist
        self.P = int(_lib.load_library().nf_param_count(C.byref(self.desc)))
        if self.P < 0:
            check(self.P)
        dev = torch.device(device)
        self.theta = theta if theta is not None else torch.zeros(self.P, dtype=dtype, device=dev)
        if self.theta.numel() != self.P:
            raise NFHipError(f"theta has {self.theta.numel()} entries, flow has {self.P} parameters")
        self.transform = Transform(self)

    # Optimisers.destructure(flow) -> (theta_flat, re)
    def destructure(self):
        def re(theta):
            return self.with_theta(theta)

        return self.theta.clone(), re

    def with_theta(self, theta: torch.Tensor) -> "Flow":
        return Flow(self.kind, self.dist, self.nlayers, self.hdims, self.K, self.B, self.theta.dtype,
                    self.theta.device, theta, self.score)

    @property
    def ctx(self):
        return context_for(self.theta.device)


class CompositeFlow(Flow):
    """create_flow((L1, ..., Ln), q0) with bijectors of different families (src/flows/utils.jl:23-26: any list of
    bijectors composes).  `segments` are single-family flows in flat order (the first is the outermost = applied
    last); theta is their thetas concatenated -- the order Optimisers.destructure walks the composition."""

    def __init__(self, segments: Sequence[Flow], dist: MvNormal, theta: Optional[torch.Tensor] = None):
        if not segments:
            raise NFHipError("create_flow: empty layer list")
        dt, dev = segments[0].theta.dtype, segments[0].theta.device
        for f in segments:
            if isinstance(f, CompositeFlow) or f.kind in ("hamiltonian", "preconditioned", "noncentred"):
                raise NFHipError("create_flow: segments must be single-family flows")
            if f.kind == "fullrank":
                raise NFHipError("create_flow: a full-rank Shift o Scale(LowerTriangular) is not built as a segment yet")
            if f.dist.d != dist.d or f.theta.dtype != dt or f.theta.device != dev:
                raise NFHipError("create_flow: every layer must share the dimension, element type and device")
        self.kind, self.dist, self.nlayers = "composite", dist, 1
        self.hdims, self.K, self.B, self.score = (), 0, 0.0, None
        self.segments = list(segments)
        self._seg_descs = (FlowDesc * len(segments))()
        for i, f in enumerate(segments):
            C.memmove(C.addressof(self._seg_descs[i]), C.addressof(f.desc), C.sizeof(FlowDesc))
            self._seg_descs[i].base = None  # q0 belongs to the composition
        self.desc = FlowDesc()
        self.desc.kind = _lib.NF_KIND["composite"]
        self.desc.dtype = _dtype_code(dt)
        self.desc.d = dist.d
        self.desc.nlayers = 1
        self.desc.nsegments = len(segments)
        self.desc.segments = C.addressof(self._seg_descs)
        if not dist.standard:
            if dist.mu.dtype != dt:
                raise NFHipError(f"base distribution is {dist.mu.dtype}, flow parameters are {dt}")
            self.desc.base = C.addressof(dist.c)
        self.P = int(_lib.load_library().nf_param_count(C.byref(self.desc)))
        if self.P < 0:
            check(self.P)
        self.theta = theta if theta is not None else torch.cat([f.theta for f in segments])
        if self.theta.numel() != self.P:
            raise NFHipError(f"theta has {self.theta.numel()} entries, flow has {self.P} parameters")
        self.transform = Transform(self)

    def with_theta(self, theta: torch.Tensor) -> "CompositeFlow":
        return CompositeFlow(self.segments, self.dist, theta)


class PrecondFlow(Flow):
    """transformed(q0, Shift(mu) o Scale(LowerTriangular(L)) o couplings): `inner` (a realnvp / nsf flow) under a full-rank
    affine layer, one family of its own (NF_KIND_PRECOND).  theta = [mu (d) ; L, d x d column-major ; inner.theta], outermost
    first; flat layer order 0 = Shift, 1 = Scale, 2... = the couplings."""

    def __init__(self, inner: Flow, dist: MvNormal, theta: torch.Tensor):
        if isinstance(inner, (CompositeFlow, PrecondFlow)) or inner.kind not in ("realnvp", "nsf"):
            raise NFHipError("preconditioned: the inner flow must be a realnvp or nsf flow")
        if inner.dist.d != dist.d:
            raise NFHipError("preconditioned: the inner flow and q0 must share the dimension")
        dt = inner.theta.dtype
        self.kind, self.dist, self.nlayers = "preconditioned", dist, 1
        self.hdims, self.K, self.B, self.score = (), 0, 0.0, None
        self.inner = inner
        self._inner_desc = FlowDesc()
        C.memmove(C.addressof(self._inner_desc), C.addressof(inner.desc), C.sizeof(FlowDesc))
        self._inner_desc.base = None  # q0 belongs to the outer flow
        self.desc = FlowDesc()
        self.desc.kind = _lib.NF_KIND["preconditioned"]
        self.desc.dtype = _dtype_code(dt)
        self.desc.d = dist.d
        self.desc.nlayers = 1
        self.desc.nsegments = 1
        self.desc.segments = C.addressof(self._inner_desc)
        if not dist.standard:
            if dist.mu.dtype != dt:
                raise NFHipError(f"base distribution is {dist.mu.dtype}, flow parameters are {dt}")
            self.desc.base = C.addressof(dist.c)
        self.P = int(_lib.load_library().nf_param_count(C.byref(self.desc)))
        if self.P < 0:
            check(self.P)
        self.theta = theta
        if self.theta.numel() != self.P:
            raise NFHipError(f"theta has {self.theta.numel()} entries, flow has {self.P} parameters")
        self.transform = Transform(self)

    def with_theta(self, theta: torch.Tensor) -> "PrecondFlow":
        return PrecondFlow(self.inner, self.dist, theta)


def preconditioned(inner: Flow, *, mu: Optional[torch.Tensor] = None, L: Optional[torch.Tensor] = None,
                   init: Optional[Flow] = None) -> Flow:
    """create_flow((Shift(mu), Scale(LowerTriangular(L)), couplings...), q0) as one family: y = mu + L T_inner(x) on the
    inner flow's q0.  Default mu = 0, L = I (forward and logpdf then equal the inner flow's to rounding); `L` is the d x d
    matrix (row i, column k at L[i, k]; what lies above the diagonal is kept in theta and never read).  `init=` takes a
    `fullrank` flow of the same d and element type and copies its [mu ; L] bit for bit: fit full-rank ADVI, then refine."""
    if not isinstance(inner, Flow) or isinstance(inner, (CompositeFlow, PrecondFlow)) or inner.kind not in ("realnvp", "nsf"):
        raise NFHipError("preconditioned: the inner flow must be a realnvp or nsf flow")
    d, dt, dev = inner.dist.d, inner.theta.dtype, inner.theta.device
    if init is not None:
        if mu is not None or L is not None:
            raise NFHipError("preconditioned: give init= or mu= / L=, not both")
        if not isinstance(init, Flow) or init.kind != "fullrank" or init.dist.d != d or init.theta.dtype != dt:
            raise NFHipError("preconditioned: init= must be a fullrank flow of the same dimension and element type")
        head = init.theta.detach().to(dev).clone()
    else:
        mu = torch.zeros(d, dtype=dt, device=dev) if mu is None else mu
        L = torch.eye(d, dtype=dt, device=dev) if L is None else L
        if mu.shape != (d,) or L.shape != (d, d):
            raise NFHipError(f"preconditioned: mu must be ({d},) and L ({d}, {d})")
        head = torch.cat([mu.to(dt).to(dev), L.to(dt).to(dev).t().contiguous().reshape(-1)])  # column-major
    return PrecondFlow(inner, inner.dist, torch.cat([head, inner.theta.detach()]))


class NoncentredFlow(Flow):
    """transformed(q0, S o T): `inner` (a realnvp, nsf or fullrank flow) under the non-centring layer S of a hierarchical target
    (NF_KIND_NONCENTRED).  theta = [lam (p) ; inner.theta]; `lam` and `inner` are views of it.  Flat layer order: the inner flow's
    layers first, S last.  The flow keeps `target`: S reads the groups from its device buffer."""

    def __init__(self, inner: Flow, target, dist: MvNormal, theta: torch.Tensor, learn: bool = True):
        if isinstance(inner, (CompositeFlow, PrecondFlow, NoncentredFlow)) or inner.kind not in ("realnvp", "nsf", "fullrank"):
            raise NFHipError("noncentred: the inner flow must be a realnvp, nsf or fullrank flow")
        if inner.dist.d != dist.d:
            raise NFHipError("noncentred: the inner flow and q0 must share the dimension")
        if not isinstance(target, (HierarchicalGLMTarget, DispersionGLMTarget)):
            raise NFHipError("noncentred: the target must be a HierarchicalGLMTarget or a DispersionGLMTarget")
        dt = inner.theta.dtype
        check_target(target, dt, inner.theta.device, dist.d)
        self.kind, self.dist, self.nlayers = "noncentred", dist, 1
        self.hdims, self.K, self.B, self.score = (), 0 if learn else 1, 0.0, target
        self.learn = bool(learn)
        self._inner_desc = FlowDesc()
        C.memmove(C.addressof(self._inner_desc), C.addressof(inner.desc), C.sizeof(FlowDesc))
        self._inner_desc.base = None  # q0 belongs to the outer flow
        self.desc = FlowDesc()
        self.desc.kind = _lib.NF_KIND["noncentred"]
        self.desc.dtype = _dtype_code(dt)
        self.desc.d = dist.d
        self.desc.nlayers = 1
        self.desc.K = self.K
        self.desc.score = C.addressof(target.c)
        self.desc.nsegments = 1
        self.desc.segments = C.addressof(self._inner_desc)
        if not dist.standard:
            if dist.mu.dtype != dt:
                raise NFHipError(f"base distribution is {dist.mu.dtype}, flow parameters are {dt}")
            self.desc.base = C.addressof(dist.c)
        self.P = int(_lib.load_library().nf_param_count(C.byref(self.desc)))
        if self.P < 0:
            check(self.P)
        self.theta = theta
        if self.theta.numel() != self.P:
            raise NFHipError(f"theta has {self.theta.numel()} entries, flow has {self.P} parameters")
        self.lam = self.theta[:target.p]
        self.inner = inner.with_theta(self.theta[target.p:])
        self.transform = Transform(self)

    def with_theta(self, theta: torch.Tensor) -> "NoncentredFlow":
        return NoncentredFlow(self.inner, self.score, self.dist, theta, self.learn)


def noncentred(inner: Flow, target, *, lam=1.0, learn: bool = True) -> Flow:
    """The inner flow under the non-centring layer of `target` (a HierarchicalGLMTarget or DispersionGLMTarget, centred as it is):
    over z = [beta ; tau (; lambda)], y_j = z_j exp(lam_j tau_g(j)) for every coefficient j with a group g(j), every other
    coordinate unchanged.  lam = 0 is the identity, lam = 1 the non-centred parameterisation beta = exp(tau) z; `lam` is a scalar
    or a (p,) tensor and is trained with the flow unless learn=False (its gradient entries are then exactly 0)."""
    if not isinstance(target, (HierarchicalGLMTarget, DispersionGLMTarget)):
        raise NFHipError("noncentred: the target must be a HierarchicalGLMTarget or a DispersionGLMTarget")
    if not isinstance(inner, Flow):
        raise NFHipError("noncentred: the inner flow must be a realnvp, nsf or fullrank flow")
    dt, dev, p = inner.theta.dtype, inner.theta.device, target.p
    if isinstance(lam, torch.Tensor) and lam.dim() > 0:
        if lam.shape != (p,):
            raise NFHipError(f"noncentred: lam must be a scalar or ({p},)")
        head = lam.detach().to(dt).to(dev).clone()
    else:
        head = torch.full((p,), float(lam), dtype=dt, device=dev)
    return NoncentredFlow(inner, target, inner.dist, torch.cat([head, inner.theta.detach()]), learn)


def create_flow(Ls: Sequence[Flow], q0: MvNormal) -> Flow:
    """create_flow(Ls, q0) = transformed(q0, reduce(o, Ls))  (src/flows/utils.jl:23-26).  `Ls` are flows built by the
    constructors below (each contributes its transform); one element returns that flow on q0, several compose."""
    Ls = list(Ls)
    if len(Ls) == 1 and not isinstance(Ls[0], CompositeFlow) and Ls[0].dist is q0:
        return Ls[0]
    return CompositeFlow(Ls, q0)


def inverse(t: Transform) -> Transform:
    """Bijectors.inverse"""
    return Transform(t.flow, not t.inverted, t.layer)


def layer(flow: Flow, index: int) -> Transform:
    """The `index`-th bijector of the composition in FLAT order (0 = outermost = applied last)."""
    return Transform(flow, False, index)


def with_logabsdet_jacobian(t: Transform, x: torch.Tensor):
    """Bijectors.with_logabsdet_jacobian(t, x) -> (y, logabsdetjac)
    (src/flows/realnvp.jl:69-110, src/flows/neuralspline.jl:94-140; ComposedFunction recursion
    reached from src/objectives/elbo.jl:67)."""
    flow = t.flow
    xm, vec = as_batch(x.to(flow.theta.dtype))
    d, n = xm.shape
    if d != flow.dist.d:
        raise NFHipError(f"dimension mismatch: flow has d={flow.dist.d}, input has {d}")
    y = new_batch(d, n, xm.dtype, xm.device)
    ladj = torch.empty(n, dtype=xm.dtype, device=xm.device)
    ctx = flow.ctx
    if t.layer is None:
        fn = ctx.lib.nf_flow_inv if t.inverted else ctx.lib.nf_flow_fwd
        check(fn(ctx.ptr, C.byref(flow.desc), _ptr(flow.theta), _ptr(xm), n, _ptr(y), _ptr(ladj)))
    else:
        check(ctx.lib.nf_layer_apply(ctx.ptr, C.byref(flow.desc), t.layer, int(t.inverted), _ptr(flow.theta), _ptr(xm),
                                     n, _ptr(y), _ptr(ladj)))
    if vec:
        return y[:, 0], ladj[0]
    return y, ladj


def rrule_with_logabsdet_jacobian(t: Transform, x: torch.Tensor):
    """ChainRulesCore.rrule(with_logabsdet_jacobian, t, x) -> ((y, logabsdetjac), pullback): the forward keeps its tape in
    a device buffer owned by the returned closure (nf_flow_fwd_keep), `pullback(ybar, lbar) -> (xbar, gtheta)` consumes it
    (nf_flow_bwd_kept).  This is what lets an arbitrary `logp` closure train through the library: the user's AD supplies
    ybar, the tape supplies the forward's own activations (the reference: Zygote on the forward's tape,
    src/optimize.jl:12-14; the rrule mechanism MonotonicSplines uses, test/ad.jl:126-127).  Whole forward transforms
    only (no Inverse, no single layer)."""
    flow = t.flow
    if t.inverted or t.layer is not None:
        raise NFHipError("rrule_with_logabsdet_jacobian: whole forward transform only")
    xm, vec = as_batch(x.to(flow.theta.dtype))
    d, n = xm.shape
    if d != flow.dist.d:
        raise NFHipError(f"dimension mismatch: flow has d={flow.dist.d}, input has {d}")
    dt, dev = xm.dtype, xm.device
    ctx = flow.ctx
    nbytes = int(ctx.lib.nf_tape_bytes(ctx.ptr, C.byref(flow.desc), n))
    if nbytes < 0:
        check(nbytes)
    tape = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)  # torch allocations are 512-byte aligned
    y = new_batch(d, n, dt, dev)
    ladj = torch.empty(n, dtype=dt, device=dev)
    theta = flow.theta
    check(ctx.lib.nf_flow_fwd_keep(ctx.ptr, C.byref(flow.desc), _ptr(theta), _ptr(xm), n, _ptr(y), _ptr(ladj), _ptr(tape),
                                   nbytes))

    def pullback(ybar: torch.Tensor, lbar: torch.Tensor, want_xbar: bool = True):
        """(xbar, gtheta); want_xbar=False returns (None, gtheta) and skips the cotangent's layout conversion where the
        library allows it (the reverse-KL loss does not differentiate through the base draws, src/objectives/elbo.jl:94)."""
        yb, _ = as_batch(ybar.to(dt))
        lb = lbar.to(dt).reshape(-1).contiguous()
        g = torch.empty(flow.P, dtype=dt, device=dev)
        c = flow.ctx
        if not want_xbar:
            code = c.lib.nf_flow_bwd_kept(c.ptr, C.byref(flow.desc), _ptr(theta), _ptr(tape), nbytes, _ptr(yb), _ptr(lb), n,
                                          _ptr(None), _ptr(g))
            if code == 0:
                return None, g
            if code != -1:  # NF_ERR_ARG: this flow needs the buffer (composition, or not on the tiled kernels)
                check(code)
        xbar = new_batch(d, n, dt, dev)
        check(c.lib.nf_flow_bwd_kept(c.ptr, C.byref(flow.desc), _ptr(theta), _ptr(tape), nbytes, _ptr(yb), _ptr(lb), n,
                                     _ptr(xbar), _ptr(g)))
        return (xbar[:, 0] if vec else xbar) if want_xbar else None, g

    if vec:
        return (y[:, 0], ladj[0]), pullback
    return (y, ladj), pullback


def transform(t: Transform, x: torch.Tensor):
    """Bijectors.transform(t, x)"""
    return with_logabsdet_jacobian(t, x)[0]


def base_logpdf(dist: MvNormal, xs: torch.Tensor):
    """logpdf(q0, xs) per column (MvNormal(zeros, I) or a general MvNormal(mu, Sigma))"""
    xm, vec = as_batch(xs)
    d, n = xm.shape
    if d != dist.d:
        raise NFHipError(f"dimension mismatch: distribution has d={dist.d}, input has {d}")
    if not dist.standard and dist.mu.dtype != xm.dtype:
        raise NFHipError(f"base distribution is {dist.mu.dtype}, input is {xm.dtype}")
    out = torch.empty(n, dtype=xm.dtype, device=xm.device)
    ctx = context_for(xm.device)
    check(ctx.lib.nf_base_logpdf_general(ctx.ptr, _dtype_code(xm.dtype), dist.base_ptr(), d, n, _ptr(xm), _ptr(out)))
    return out[0] if vec else out


def logpdf(flow, ys: torch.Tensor):
    """logpdf(td, y) = logpdf(td.dist, x) + ladj_inv  (Bijectors; used by
    src/objectives/loglikelihood.jl:23,31 and test/flow.jl:15)."""
    if isinstance(flow, MvNormal):
        return base_logpdf(flow, ys)
    ym, vec = as_batch(ys.to(flow.theta.dtype))
    d, n = ym.shape
    if d != flow.dist.d:
        raise NFHipError(f"dimension mismatch: flow has d={flow.dist.d}, input has {d}")
    out = torch.empty(n, dtype=ym.dtype, device=ym.device)
    val = C.c_double(0.0)
    ctx = flow.ctx
    check(ctx.lib.nf_loglikelihood(ctx.ptr, C.byref(flow.desc), _ptr(flow.theta), _ptr(ym), n, _ptr(out), C.byref(val)))
    return out[0] if vec else out


def rand(flow, n: Optional[int] = None, rng: Optional[PhiloxRNG] = None):
    """rand(rng, flow, n): base draws pushed through the transform (batched)."""
    rng = rng if rng is not None else _default_rng
    if isinstance(flow, MvNormal):
        return device_specific_rand(rng, flow, n)
    return device_specific_rand(rng, flow, n)


_default_rng = PhiloxRNG(0)


# --------------------------------------------------------------------------------------
# constructors (parameter initialisation follows the reference's init distributions:
# Flux.Dense Glorot-uniform weights / zero bias; PlanarLayer / RadialLayer randn)
# --------------------------------------------------------------------------------------
def _mlp_shapes(nin, hdims, nout):
    dims = [nin] + list(hdims) + [nout]
    return list(zip(dims[:-1], dims[1:]))


def _init_couplings(flow: Flow, gen: torch.Generator, outs_per_c):
    d = flow.dist.d
    parts = []
    for _ in range(flow.nlayers):
        for start in (0, 1):  # mask 1:2:d then 2:2:d (src/flows/realnvp.jl:138-139)
            c = len(range(start, d, 2))
            m = d - c
            for nout in outs_per_c(c):
                for (a, b) in _mlp_shapes(m, flow.hdims, nout):
                    lim = math.sqrt(6.0 / (a + b))
                    w = (torch.rand(a * b, generator=gen, dtype=torch.float64) * 2 - 1) * lim
                    parts += [w, torch.zeros(b, dtype=torch.float64)]
    return torch.cat(parts)


def _finish(flow: Flow, theta64: torch.Tensor) -> Flow:
    assert theta64.numel() == flow.P, (theta64.numel(), flow.P)
    flow.theta = theta64.to(flow.theta.dtype).to(flow.theta.device)
    return flow


def realnvp(q0: MvNormal, hdims: Sequence[int] = (32, 32), nlayers: int = 10, *, paramtype=torch.float64,
            device="cuda", seed: int = 0) -> Flow:
    """realnvp(q0, hdims, nlayers; paramtype)  (src/flows/realnvp.jl:170-192)."""
    flow = Flow("realnvp", q0, nlayers, hdims, dtype=paramtype, device=device)
    gen = torch.Generator().manual_seed(seed)
    return _finish(flow, _init_couplings(flow, gen, lambda c: (c, c)))


def nsf(q0: MvNormal, hdims: Sequence[int] = (32, 32), K: int = 10, B: float = 30.0, nlayers: int = 10, *,
        paramtype=torch.float64, device="cuda", seed: int = 0) -> Flow:
    """nsf(q0, hdims, K, B, nlayers; paramtype)  (src/flows/neuralspline.jl:218-234)."""
    flow = Flow("nsf", q0, nlayers, hdims, K, B, dtype=paramtype, device=device)
    gen = torch.Generator().manual_seed(seed)
    return _finish(flow, _init_couplings(flow, gen, lambda c: ((3 * K - 1) * c,)))


def planarflow(q0: MvNormal, nlayers: int, *, paramtype=torch.float64, device="cuda", seed: int = 0) -> Flow:
    """planarflow(q0, nlayers; paramtype)  (src/flows/planar_radial.jl:21-29)."""
    flow = Flow("planar", q0, nlayers, dtype=paramtype, device=device)
    gen = torch.Generator().manual_seed(seed)
    return _finish(flow, torch.randn(flow.P, generator=gen, dtype=torch.float64))


def radialflow(q0: MvNormal, nlayers: int, *, paramtype=torch.float64, device="cuda", seed: int = 0) -> Flow:
    """radialflow(q0, nlayers; paramtype)  (src/flows/planar_radial.jl:52-60)."""
    flow = Flow("radial", q0, nlayers, dtype=paramtype, device=device)
    gen = torch.Generator().manual_seed(seed)
    return _finish(flow, torch.randn(flow.P, generator=gen, dtype=torch.float64))


def meanfield(q0: MvNormal, *, paramtype=torch.float64, device="cuda") -> Flow:
    """transformed(q0, Shift(zeros) o Scale(ones))  (test/interface.jl:22-25)."""
    flow = Flow("meanfield", q0, 1, dtype=paramtype, device=device)
    d = q0.d
    return _finish(flow, torch.cat([torch.zeros(d, dtype=torch.float64), torch.ones(d, dtype=torch.float64)]))


def fullrank(q0: MvNormal, *, paramtype=torch.float64, device="cuda") -> Flow:
    """transformed(q0, Shift(zeros) o Scale(LowerTriangular(I))): the full-rank Gaussian family (the Shift o Scale of
    test/interface.jl:22-25 with a matrix scale).  theta = [mu(d) ; L, d x d column-major]; the strict upper triangle of
    L is part of theta and is never read by the library."""
    flow = Flow("fullrank", q0, 1, dtype=paramtype, device=device)
    d = q0.d
    return _finish(flow, torch.cat([torch.zeros(d, dtype=torch.float64), torch.eye(d, dtype=torch.float64).reshape(-1)]))


def hamiltonianflow(dims: int, nblocks: int, nleapfrog: int, target, *, logeps0: float = math.log(0.05),
                    paramtype=torch.float64, device="cuda") -> Flow:
    """The Hamiltonian flow of example/demo_hamiltonian_flow.jl:132-146 on the joint z = [x; rho] (2*dims):
    a mean-field Gaussian reference, then `nblocks` blocks (momentum Shift o Scale) o LeapFrog(dims, logeps0,
    nleapfrog, score(target)).  `target` is a built-in target of dimension `dims` (diagonal Gaussian, Banana,
    Funnel -- the ones with a closed-form Hessian-vector product); pass the same object as `logp` to
    elbo / train_flow: the library forms logp_joint(z) = logp(x) + log N(rho; 0, I) (demo :121-128)."""
    check_target(target, paramtype, device, dims)
    flow = Flow("hamiltonian", MvNormal(2 * dims), nblocks, K=nleapfrog, dtype=paramtype, device=device, score=target)
    th = [torch.zeros(2 * dims, dtype=torch.float64), torch.ones(2 * dims, dtype=torch.float64)]
    for _ in range(nblocks):
        th += [torch.zeros(dims, dtype=torch.float64), torch.ones(dims, dtype=torch.float64),
               torch.full((dims,), float(logeps0), dtype=torch.float64)]
    return _finish(flow, torch.cat(th))


# --------------------------------------------------------------------------------------
# built-in targets (the `logp` closures of the reference's tests / demos)
# --------------------------------------------------------------------------------------
class DiagGaussTarget:
    """logp(z) = logpdf(MvNormal(mu, Diagonal(var)), z)  (test/flow.jl:43-46)."""

    def __init__(self, mu: torch.Tensor, var: torch.Tensor):
        if mu.dtype != var.dtype or mu.device != var.device or mu.shape != var.shape or mu.dim() != 1:
            raise NFHipError("DiagGaussTarget: mu and var must be vectors of one length, element type and device")
        self.mu, self.var = mu.contiguous(), var.contiguous()
        self.c = Target(_lib.NF_TARGET_DIAGGAUSS, self.mu.data_ptr(), self.var.data_ptr(), 0.0, 0.0)

    def check_compatible(self, dtype, device, d=None):
        """The C ABI passes mu / var as untyped device pointers that the kernels read in the FLOW's element type:
        a Float32 target under a Float64 flow would be read out of bounds.  Refuse instead."""
        if self.mu.dtype != dtype:
            raise NFHipError(f"target parameters are {self.mu.dtype} but the flow computes in {dtype}: "
                             "build the target in the flow's element type (the reference's logp closure would promote; "
                             "the device kernels cannot)")
        dv = torch.device(device)
        if self.mu.device.type != dv.type or (dv.index is not None and self.mu.device.index is not None and dv.index != self.mu.device.index):
            raise NFHipError(f"target parameters live on {self.mu.device}, the flow on {device}")
        if d is not None and self.mu.numel() != d:
            raise NFHipError(f"target has dimension {self.mu.numel()}, expected {d}")

    def __call__(self, ys):
        return target_logp(self, ys)


class BananaTarget:
    """Banana(d, b, var)  (example/targets/banana.jl; demo_planar_flow.jl:16)."""

    def __init__(self, d: int, b: float, var: float):
        self.d, self.b, self.variance = d, float(b), float(var)
        self.c = Target(_lib.NF_TARGET_BANANA, 0, 0, self.b, self.variance)

    def __call__(self, ys):
        return target_logp(self, ys)


class FunnelTarget:
    """Funnel(d, mu, sigma)  (example/targets/neal_funnel.jl:26-44; default Funnel(d) = Funnel(d, 0, 9))."""

    def __init__(self, d: int, mu: float = 0.0, sigma: float = 9.0):
        if d < 2:
            raise ValueError("dim must be >= 2")  # neal_funnel.jl:32
        if not sigma > 0:
            raise ValueError("σ must be > 0")  # neal_funnel.jl:33
        self.d, self.mu, self.sigma = d, float(mu), float(sigma)
        self.c = Target(_lib.NF_TARGET_FUNNEL, 0, 0, self.mu, self.sigma)

    def __call__(self, ys):
        return target_logp(self, ys)


class WarpedGaussTarget:
    """WarpedGauss(σ1, σ2), 2-dimensional  (example/targets/warped_gaussian.jl:25-37; default (1.0, 0.12))."""

    def __init__(self, sigma1: float = 1.0, sigma2: float = 0.12):
        if not (sigma1 > 0 and sigma2 > 0):
            raise ValueError("σ₁, σ₂ must be > 0")  # warped_gaussian.jl:31-32
        self.d, self.sigma1, self.sigma2 = 2, float(sigma1), float(sigma2)
        self.c = Target(_lib.NF_TARGET_WARPED, 0, 0, self.sigma1, self.sigma2)

    def __call__(self, ys):
        return target_logp(self, ys)


class CrossTarget:
    """Cross(μ, σ), 2-dimensional 4-component mixture  (example/targets/cross.jl:29-38; default (2.0, 0.15))."""

    def __init__(self, mu: float = 2.0, sigma: float = 0.15):
        if not sigma > 0:
            raise ValueError("σ must be > 0")
        self.d, self.mu, self.sigma = 2, float(mu), float(sigma)
        self.c = Target(_lib.NF_TARGET_CROSS, 0, 0, self.mu, self.sigma)

    def __call__(self, ys):
        return target_logp(self, ys)


class _LinpredLogp(torch.autograd.Function):
    """logp(ys) of a linear-predictor target as a torch-autograd node whose backward is the DEVICE score
    (nf_target_logp with the gradient): what the closure branch of value_and_gradient differentiates."""

    @staticmethod
    def forward(ctx, target, ys):
        lp, grad = target_logp(target, ys.detach(), with_grad=True)
        ctx.save_for_backward(grad)
        ctx.vec = ys.dim() == 1
        return lp

    @staticmethod
    def backward(ctx, lbar):
        (grad,) = ctx.saved_tensors
        g = grad[:, 0] * lbar if ctx.vec else grad * lbar.unsqueeze(0)
        return None, g


class _LinpredTarget:
    """What MvNormalTarget, LogisticRegressionTarget, MixtureTarget, the GLM targets and SoftmaxRegressionTarget share: the matrix `A` [rows, d] and the optional shift `mu`,
    kept alive for the descriptor's device pointers, and the checks DiagGaussTarget makes (the ABI reads p0 / p1 untyped)."""

    def check_compatible(self, dtype, device, d=None):
        if self.A.dtype != dtype:
            raise NFHipError(f"target parameters are {self.A.dtype} but the flow computes in {dtype}: "
                             "build the target in the flow's element type")
        dv = torch.device(device)
        if self.A.device.type != dv.type or (dv.index is not None and self.A.device.index is not None and dv.index != self.A.device.index):
            raise NFHipError(f"target parameters live on {self.A.device}, the flow on {device}")
        if d is not None and self.d != d:
            raise NFHipError(f"target has dimension {self.d}, expected {d}")

    def __call__(self, ys):
        if ys.requires_grad:
            return _LinpredLogp.apply(self, ys)
        return target_logp(self, ys)


class MvNormalTarget(_LinpredTarget):
    """logp(z) = logpdf(MvNormal(mu, Sigma), z) with a full covariance (the correlated form of test/flow.jl:43-46).
    Sigma = L L' is factored on the host in float64; the device reads W = inv(L), u = W (z - mu) ~ N(0, I)."""

    def __init__(self, mu: torch.Tensor, Sigma: torch.Tensor):
        if mu.dim() != 1 or Sigma.dim() != 2 or Sigma.shape != (mu.numel(), mu.numel()):
            raise NFHipError("MvNormalTarget: mu (d,), Sigma (d, d)")
        if mu.dtype != Sigma.dtype or mu.device != Sigma.device or mu.dtype not in (torch.float32, torch.float64):
            raise NFHipError("MvNormalTarget: mu and Sigma must share one element type (Float32 or Float64) and one device")
        S64 = Sigma.detach().to("cpu", torch.float64)
        if not bool(torch.isfinite(S64).all()) or not torch.allclose(S64, S64.T, rtol=1e-6, atol=1e-12 * float(S64.abs().max() + 1)):
            raise NFHipError("MvNormalTarget: Sigma is not symmetric")
        L, info = torch.linalg.cholesky_ex(S64)
        if int(info) != 0:
            raise NFHipError("MvNormalTarget: Sigma is not positive definite")
        d = mu.numel()
        W64 = torch.linalg.solve_triangular(L, torch.eye(d, dtype=torch.float64), upper=False)
        self.d = d
        self.mu = mu.detach().contiguous()
        self.A = torch.tril(W64).to(mu.dtype).to(mu.device).contiguous()
        self.W = self.A
        self.logdet_w = float(-torch.log(torch.diagonal(L)).sum())
        self.c = Target(_lib.NF_TARGET_DENSEGAUSS, self.mu.data_ptr(), self.A.data_ptr(), self.logdet_w, 0.0)


class LogisticRegressionTarget(_LinpredTarget):
    """Posterior of Bayesian logistic regression over the weights z in R^d: data rows X [n, d], labels t in {-1, +1} (or
    {0, 1}, mapped to them), prior N(0, prior_sigma^2 I):
        logp(z) = sum_i log sigmoid(t_i x_i . (z - shift)) - |z|^2 / (2 prior_sigma^2) - d/2 log(2 pi prior_sigma^2).
    The labels are folded into the rows on the host (A_i = t_i x_i)."""

    def __init__(self, X: torch.Tensor, t: torch.Tensor, prior_sigma: float = 1.0, shift: torch.Tensor = None):
        if X.dim() != 2 or X.shape[0] < 1 or X.shape[1] < 1 or X.dtype not in (torch.float32, torch.float64):
            raise NFHipError("LogisticRegressionTarget: X must be a Float32 or Float64 matrix [n, d] with n >= 1")
        n, d = X.shape
        if t.dim() != 1 or t.numel() != n:
            raise NFHipError("LogisticRegressionTarget: one label per row of X")
        if not prior_sigma > 0:
            raise NFHipError("LogisticRegressionTarget: prior_sigma must be > 0")
        tv = t.detach().to("cpu", torch.float64)
        if bool(((tv == 1) | (tv == -1)).all()):
            sign = tv
        elif bool(((tv == 0) | (tv == 1)).all()):
            sign = 2.0 * tv - 1.0
        else:
            raise NFHipError("LogisticRegressionTarget: labels must all be in {-1, +1} or all in {0, 1}")
        if shift is not None and (shift.dim() != 1 or shift.numel() != d or shift.dtype != X.dtype or shift.device != X.device):
            raise NFHipError("LogisticRegressionTarget: shift must be a vector (d,) of X's element type and device")
        self.d, self.n, self.prior_sigma = d, n, float(prior_sigma)
        self.A = (X.detach() * sign.to(X.dtype).to(X.device).unsqueeze(1)).contiguous()
        self.mu = shift.detach().contiguous() if shift is not None else None
        self.c = Target(_lib.NF_TARGET_LOGREG, self.mu.data_ptr() if self.mu is not None else 0, self.A.data_ptr(), float(n),
                        self.prior_sigma)


class MixtureTarget(_LinpredTarget):
    """logp(z) = logpdf(MixtureModel([MvNormal(mus[k], Sigmas[k]) for k], weights), z): K full-covariance Gaussians
    (example/targets/cross.jl:31-37 builds Cross this way).  weights (K,), mus (K, d), Sigmas (K, d, d), one element type
    and device.  Every Sigma_k = L_k L_k' is factored on the host in float64; the device reads the W_k = inv(L_k) stacked
    (`A` [K d, d]) and one buffer `p0` = mbar | b | c with the common centre mbar = sum_k pi_k mu_k,
    b_k = W_k (mu_k - mbar) and c_k = log pi_k + log|det W_k| - d/2 log(2 pi).  Weights are renormalised in float64;
    zero-weight components are dropped."""

    def __init__(self, weights: torch.Tensor, mus: torch.Tensor, Sigmas: torch.Tensor):
        if weights.dim() != 1 or mus.dim() != 2 or Sigmas.dim() != 3 or weights.numel() < 1 or mus.shape[1] < 1 or \
                mus.shape[0] != weights.numel() or tuple(Sigmas.shape) != (mus.shape[0], mus.shape[1], mus.shape[1]):
            raise NFHipError("MixtureTarget: weights (K,), mus (K, d), Sigmas (K, d, d) with K >= 1")
        if not (weights.dtype == mus.dtype == Sigmas.dtype) or not (weights.device == mus.device == Sigmas.device) or \
                mus.dtype not in (torch.float32, torch.float64):
            raise NFHipError("MixtureTarget: weights, mus and Sigmas must share one element type (Float32 or Float64) and one device")
        w64 = weights.detach().to("cpu", torch.float64)
        if not bool(torch.isfinite(w64).all()) or bool((w64 < 0).any()) or abs(float(w64.sum()) - 1.0) > 1e-6:
            raise NFHipError("MixtureTarget: weights must be >= 0 and sum to 1 (within 1e-6)")
        w64 = w64 / w64.sum()
        keep = [k for k in range(w64.numel()) if float(w64[k]) > 0.0]
        d = mus.shape[1]
        m64 = mus.detach().to("cpu", torch.float64)
        S64 = Sigmas.detach().to("cpu", torch.float64)
        if not bool(torch.isfinite(m64).all()):
            raise NFHipError("MixtureTarget: mus must be finite")
        eye = torch.eye(d, dtype=torch.float64)
        Ws, logdets = [], []
        for k in keep:
            Sk = S64[k]
            if not bool(torch.isfinite(Sk).all()) or not torch.allclose(Sk, Sk.T, rtol=1e-6, atol=1e-12 * float(Sk.abs().max() + 1)):
                raise NFHipError(f"MixtureTarget: Sigma of component {k} is not symmetric")
            L, info = torch.linalg.cholesky_ex(Sk)
            if int(info) != 0:
                raise NFHipError(f"MixtureTarget: Sigma of component {k} is not positive definite")
            Ws.append(torch.tril(torch.linalg.solve_triangular(L, eye, upper=False)))
            logdets.append(-torch.log(torch.diagonal(L)).sum())
        pi = w64[keep]
        mk = m64[keep]
        W = torch.stack(Ws)                                     # [K, d, d]
        mbar = (pi[:, None] * mk).sum(0)
        b = torch.einsum("kij,kj->ki", W, mk - mbar[None, :])   # [K, d]
        c = torch.log(pi) + torch.stack(logdets) - 0.5 * d * math.log(2.0 * math.pi)
        self.d, self.K = d, len(keep)
        self.weights = pi
        self.A = W.reshape(self.K * d, d).to(mus.dtype).to(mus.device).contiguous()
        self.p0 = torch.cat([mbar, b.reshape(-1), c]).to(mus.dtype).to(mus.device).contiguous()
        self.c = Target(_lib.NF_TARGET_GAUSSMIX, self.p0.data_ptr(), self.A.data_ptr(), float(self.K), 0.0)


_GLM_KINDS = {"logit": _lib.NF_TARGET_GLM_LOGIT, "probit": _lib.NF_TARGET_GLM_PROBIT, "poisson": _lib.NF_TARGET_GLM_POISSON,
              "student": _lib.NF_TARGET_GLM_STUDENT, "normal": _lib.NF_TARGET_GLM_NORMAL}


def _glm_matrix(name, X):
    if not isinstance(X, torch.Tensor) or X.dim() != 2 or X.shape[0] < 1 or X.shape[1] < 1 or X.dtype not in (torch.float32, torch.float64):
        raise NFHipError(f"{name}: the data matrix must be a Float32 or Float64 tensor [rows, d] with rows >= 1 and d >= 1")
    X64 = X.detach().to("cpu", torch.float64)
    if not bool(torch.isfinite(X64).all()):
        raise NFHipError(f"{name}: the data matrix must be finite")
    return X64


def _glm_vector(name, what, v, like, n, default=None, nonneg=False, positive=False):
    """a per-row (or per-feature) vector as float64 on the host: `like`'s element type (integer tensors are taken as counts /
    labels), `like`'s device, length n, finite"""
    if v is None:
        return torch.full((n,), float(default), dtype=torch.float64)
    if not isinstance(v, torch.Tensor) or v.dim() != 1 or v.numel() != n:
        raise NFHipError(f"{name}: {what} must be a vector of length {n}")
    if v.device != like.device or (v.dtype.is_floating_point and v.dtype != like.dtype) or v.dtype.is_complex or v.dtype == torch.bool:
        raise NFHipError(f"{name}: {what} must be on the data matrix's device and of its element type (or an integer tensor)")
    v64 = v.detach().to("cpu", torch.float64)
    if not bool(torch.isfinite(v64).all()):
        raise NFHipError(f"{name}: {what} must be finite")
    if (nonneg and bool((v64 < 0).any())) or (positive and bool((v64 <= 0).any())):
        raise NFHipError(f"{name}: {what} must be {'> 0' if positive else '>= 0'}")
    return v64


def _glm_scalar(name, what, x, positive=True, allow_inf=False):
    x = float(x)
    if math.isnan(x) or (math.isinf(x) and not (allow_inf and x > 0)) or (positive and not x > 0):
        raise NFHipError(f"{name}: {what} must be a finite number" + (" > 0" if positive else "") + (" (or +inf)" if allow_inf else ""))
    return x


class GLMTarget(_LinpredTarget):
    """The generalised linear-predictor target (NF_TARGET_GLM_*), with u = A z + offset:
        logp(z) = const + sum_i weights_i phi(u_i; param) + lin . z - |z|^2 / (2 prior_sigma^2) - d/2 log(2 pi prior_sigma^2)
    family: "logit" (phi = log sigmoid), "probit" (log Phi), "poisson" (-exp), "student" (-(nu+1)/2 log1p(u^2/nu), nu = param)
    or "normal" (-u^2/2).  A [rows, d]; offset, weights (>= 0; 0 drops the row exactly) per row; lin per feature; all of A's
    element type and device.  prior_sigma = math.inf is the flat prior.  The device reads `A` and ONE buffer
    `p0` = lin | offset | weights | (param, const); both are kept alive here."""

    def __init__(self, family, A, offset=None, weights=None, lin=None, const=0.0, param=0.0, prior_sigma=1.0, _name="GLMTarget"):
        if family not in _GLM_KINDS:
            raise NFHipError(f"{_name}: family must be one of {sorted(_GLM_KINDS)}")
        A64 = _glm_matrix(_name, A)
        rows, d = A64.shape
        off = _glm_vector(_name, "offset", offset, A, rows, 0.0)
        wt = _glm_vector(_name, "weights", weights, A, rows, 1.0, nonneg=True)
        ln = _glm_vector(_name, "lin", lin, A, d, 0.0)
        const = _glm_scalar(_name, "const", const, positive=False)
        param = _glm_scalar(_name, "param", param, positive=family == "student")
        self.prior_sigma = _glm_scalar(_name, "prior_sigma", prior_sigma, allow_inf=True)
        self.family, self.d, self.rows, self.param, self.const = family, d, rows, param, const
        self.A = A.detach().contiguous()
        self.p0 = torch.cat([ln, off, wt, torch.tensor([param, const], dtype=torch.float64)]).to(A.dtype).to(A.device).contiguous()
        self.c = Target(_GLM_KINDS[family], self.p0.data_ptr(), self.A.data_ptr(), float(rows), self.prior_sigma)



class PoissonRegressionTarget(GLMTarget):
    """Posterior of Poisson regression (log link) over the weights z: counts k_i ~ Poisson(exposure_i exp(x_i . z)), prior
    N(0, prior_sigma^2 I), each row's log-likelihood under weight w_i.  Folds to the "poisson" family with A = X,
    offset = log exposure, lin = sum_i w_i k_i x_i and const = sum_i w_i (k_i offset_i - lgamma(k_i + 1))."""

    def __init__(self, X, counts, exposure=None, weights=None, prior_sigma=1.0):
        nm = "PoissonRegressionTarget"
        X64 = _glm_matrix(nm, X)
        n = X64.shape[0]
        k = _glm_vector(nm, "counts", counts, X, n, nonneg=True)
        if bool((k != torch.round(k)).any()):
            raise NFHipError(f"{nm}: counts must be integers")
        off = torch.log(_glm_vector(nm, "exposure", exposure, X, n, 1.0, positive=True))
        w = _glm_vector(nm, "weights", weights, X, n, 1.0, nonneg=True)
        lin = (w * k) @ X64
        const = float((w * (k * off - torch.lgamma(k + 1.0))).sum())
        to = lambda t: t.to(X.dtype).to(X.device)
        super().__init__("poisson", X, to(off), to(w), to(lin), const, 0.0, prior_sigma, _name=nm)


class BinomialRegressionTarget(GLMTarget):
    """Posterior of binomial (logit-link) regression: successes k_i ~ Binomial(trials n_i, sigmoid(x_i . z + offset_i)).
    With eta = x . z + offset:  k log sigmoid(eta) + (n - k) log sigmoid(-eta) = k eta + n log sigmoid(-eta), so it folds
    to the "logit" family with A = -X, offset -> -offset, weights -> w n, lin = sum_i w_i k_i x_i and
    const = sum_i w_i (k_i offset_i + log C(n_i, k_i))."""

    def __init__(self, X, successes, trials, offset=None, weights=None, prior_sigma=1.0):
        nm = "BinomialRegressionTarget"
        X64 = _glm_matrix(nm, X)
        n = X64.shape[0]
        k = _glm_vector(nm, "successes", successes, X, n, nonneg=True)
        nt = _glm_vector(nm, "trials", trials, X, n, nonneg=True)
        if bool((k != torch.round(k)).any()) or bool((nt != torch.round(nt)).any()) or bool((k > nt).any()):
            raise NFHipError(f"{nm}: successes and trials must be integers with 0 <= successes <= trials")
        off = _glm_vector(nm, "offset", offset, X, n, 0.0)
        w = _glm_vector(nm, "weights", weights, X, n, 1.0, nonneg=True)
        lin = (w * k) @ X64
        logc = torch.lgamma(nt + 1.0) - torch.lgamma(k + 1.0) - torch.lgamma(nt - k + 1.0)
        const = float((w * (k * off + logc)).sum())
        to = lambda t: t.to(X.dtype).to(X.device)
        super().__init__("logit", to(-X64), to(-off), to(w * nt), to(lin), const, 0.0, prior_sigma, _name=nm)


class ProbitRegressionTarget(GLMTarget):
    """Posterior of probit regression: P(t_i = +1) = Phi(x_i . z + offset_i); labels as LogisticRegressionTarget takes them
    ({-1, +1} or {0, 1}).  The labels are folded into the rows: A_i = t_i x_i, offset_i -> t_i offset_i."""

    def __init__(self, X, t, offset=None, weights=None, prior_sigma=1.0):
        nm = "ProbitRegressionTarget"
        X64 = _glm_matrix(nm, X)
        n = X64.shape[0]
        tv = _glm_vector(nm, "labels", t, X, n)
        if bool(((tv == 1) | (tv == -1)).all()):
            sign = tv
        elif bool(((tv == 0) | (tv == 1)).all()):
            sign = 2.0 * tv - 1.0
        else:
            raise NFHipError(f"{nm}: labels must all be in {{-1, +1}} or all in {{0, 1}}")
        off = _glm_vector(nm, "offset", offset, X, n, 0.0)
        w = _glm_vector(nm, "weights", weights, X, n, 1.0, nonneg=True)
        to = lambda t_: t_.to(X.dtype).to(X.device)
        super().__init__("probit", to(X64 * sign[:, None]), to(sign * off), to(w), None, 0.0, 0.0, prior_sigma, _name=nm)


class RobustRegressionTarget(GLMTarget):
    """Posterior of linear regression with Student-t noise: (y_i - x_i . z) / scale ~ t_nu.  Folds to the "student" family
    with A = X / scale, offset = -y / scale, param = nu and
    const = sum_i w_i (lgamma((nu+1)/2) - lgamma(nu/2) - log(nu pi)/2 - log scale)."""

    def __init__(self, X, y, nu, scale, weights=None, prior_sigma=1.0):
        nm = "RobustRegressionTarget"
        X64 = _glm_matrix(nm, X)
        n = X64.shape[0]
        yv = _glm_vector(nm, "y", y, X, n)
        nu = _glm_scalar(nm, "nu", nu)
        scale = _glm_scalar(nm, "scale", scale)
        w = _glm_vector(nm, "weights", weights, X, n, 1.0, nonneg=True)
        const = float(w.sum()) * (math.lgamma(0.5 * (nu + 1.0)) - math.lgamma(0.5 * nu) - 0.5 * math.log(nu * math.pi) - math.log(scale))
        to = lambda t: t.to(X.dtype).to(X.device)
        super().__init__("student", to(X64 / scale), to(-yv / scale), to(w), None, const, nu, prior_sigma, _name=nm)


class LinearRegressionTarget(GLMTarget):
    """Posterior of Gaussian linear regression with known noise: y_i ~ N(x_i . z, noise_sigma^2).  Folds to the "normal"
    family with A = X / noise_sigma, offset = -y / noise_sigma and const = sum_i w_i (-log(2 pi)/2 - log noise_sigma)."""

    def __init__(self, X, y, noise_sigma, weights=None, prior_sigma=1.0):
        nm = "LinearRegressionTarget"
        X64 = _glm_matrix(nm, X)
        n = X64.shape[0]
        yv = _glm_vector(nm, "y", y, X, n)
        sn = _glm_scalar(nm, "noise_sigma", noise_sigma)
        w = _glm_vector(nm, "weights", weights, X, n, 1.0, nonneg=True)
        const = float(w.sum()) * (-0.5 * math.log(2.0 * math.pi) - math.log(sn))
        to = lambda t: t.to(X.dtype).to(X.device)
        super().__init__("normal", to(X64 / sn), to(-yv / sn), to(w), None, const, 0.0, prior_sigma, _name=nm)


_HGLM_KINDS = {"logit": _lib.NF_TARGET_HGLM_LOGIT, "probit": _lib.NF_TARGET_HGLM_PROBIT, "poisson": _lib.NF_TARGET_HGLM_POISSON,
               "student": _lib.NF_TARGET_HGLM_STUDENT, "normal": _lib.NF_TARGET_HGLM_NORMAL}
_HYPER_KINDS = {"lognormal": 0, "halfnormal": 1, "halfcauchy": 2}


def _per_item(name, what, v, n, positive=False, allow_inf=False):
    """a scalar or one value per item (a sequence or tensor of length n) as float64 [n] on the host"""
    if isinstance(v, torch.Tensor) and v.dim() == 1 or isinstance(v, (list, tuple)):
        v64 = torch.as_tensor(v).detach().to("cpu", torch.float64)
        if v64.dim() != 1 or v64.numel() != n:
            raise NFHipError(f"{name}: {what} must be a scalar or hold {n} values")
    elif isinstance(v, torch.Tensor) and v.dim() > 1:
        raise NFHipError(f"{name}: {what} must be a scalar or hold {n} values")
    else:
        v64 = torch.full((n,), float(v), dtype=torch.float64)
    fin = torch.isfinite(v64) | ((v64 == math.inf) if allow_inf else torch.zeros_like(v64, dtype=torch.bool))
    if not bool(fin.all()) or (positive and bool((v64 <= 0).any())):
        raise NFHipError(f"{name}: {what} must be finite" + (" and > 0" if positive else "") + (" (or +inf)" if allow_inf else ""))
    return v64


class HierarchicalGLMTarget(_LinpredTarget):
    """A GLM posterior under a hierarchical prior (NF_TARGET_HGLM_*), over z = [beta (p coefficients) ; tau (G group log-scales)],
    d = p + G, in the centred parameterisation:
        logp(z) = const + sum_i weights_i phi(u_i; param) + lin . beta + sum_j log N(beta_j; 0, sigma_j^2) + sum_g log p(tau_g),
        u = A beta + offset,   sigma_j = fixed_sigma_j if groups[j] == -1 else exp(tau_{groups[j]}).
    family and A [rows, p], offset, weights, lin (p,), const, param are GLMTarget's.  groups: an integer tensor (p,) with values in
    {-1, 0 .. n_groups - 1}; fixed_sigma: a scalar or (p,), read where groups == -1, math.inf = a flat prior on that coefficient.
    hyper: "lognormal" (tau_g ~ N(hyper_loc, hyper_scale^2)), "halfnormal" or "halfcauchy" (exp(tau_g) ~ half-normal / half-Cauchy
    of scale hyper_scale, as a density over tau_g), one name or one per group; hyper_loc, hyper_scale: a scalar or one per group.
    Everything linear in z or constant is folded here in float64 (the -n_g tau_g of the Gaussian normalisers and the +tau_g
    Jacobian of the half-families into lin, every normaliser into the constant).  The device reads `A` (padded with zero
    tau-columns to [rows, d]) and ONE buffer `p0` (include/nfhip.h); both are kept alive here."""

    def __init__(self, family, A, groups, n_groups, offset=None, weights=None, lin=None, const=0.0, param=0.0, fixed_sigma=1.0,
                 hyper="halfcauchy", hyper_loc=0.0, hyper_scale=1.0, _name="HierarchicalGLMTarget"):
        nm = _name
        if family not in _HGLM_KINDS:
            raise NFHipError(f"{nm}: family must be one of {sorted(_HGLM_KINDS)}")
        A64 = _glm_matrix(nm, A)
        rows, p = A64.shape
        if isinstance(n_groups, bool) or not hasattr(n_groups, "__index__") or int(n_groups) < 0:
            raise NFHipError(f"{nm}: n_groups must be an integer >= 0")
        G = int(n_groups)
        d = p + G
        if d > 256:
            raise NFHipError(f"{nm}: p + n_groups = {d} exceeds the kernels' d = 256")
        if not isinstance(groups, torch.Tensor) or groups.dim() != 1 or groups.numel() != p or groups.dtype.is_floating_point or \
                groups.dtype.is_complex or groups.dtype == torch.bool:
            raise NFHipError(f"{nm}: groups must be an integer tensor of length {p}")
        grp = groups.detach().to("cpu", torch.int64)
        if bool((grp < -1).any()) or bool((grp >= G).any()):
            raise NFHipError(f"{nm}: groups must hold -1 (a fixed prior scale) or a group index in 0..{G - 1}")
        off = _glm_vector(nm, "offset", offset, A, rows, 0.0)
        wt = _glm_vector(nm, "weights", weights, A, rows, 1.0, nonneg=True)
        ln = _glm_vector(nm, "lin", lin, A, p, 0.0)
        const = _glm_scalar(nm, "const", const, positive=False)
        param = _glm_scalar(nm, "param", param, positive=family == "student")
        sig = _per_item(nm, "fixed_sigma", fixed_sigma, p, positive=True, allow_inf=True)
        names = [hyper] * G if isinstance(hyper, str) else list(hyper)
        if len(names) != G or any(not isinstance(h, str) or h not in _HYPER_KINDS for h in names):
            raise NFHipError(f"{nm}: hyper must be one of {sorted(_HYPER_KINDS)}, or one of them per group")
        loc = _per_item(nm, "hyper_loc", hyper_loc, G)
        scl = _per_item(nm, "hyper_scale", hyper_scale, G, positive=True)

        grouped = grp >= 0
        isd = torch.where(grouped, torch.zeros(p, dtype=torch.float64), 1.0 / sig)        # 1 / inf = 0: flat
        n_g = torch.bincount(grp[grouped], minlength=G).to(torch.float64) if G else torch.zeros(0, dtype=torch.float64)
        L2PI = math.log(2.0 * math.pi)
        fixed = (~grouped) & torch.isfinite(sig)
        c = const - float(torch.log(sig[fixed]).sum()) - 0.5 * L2PI * float(fixed.sum()) - 0.5 * L2PI * float(grouped.sum())
        hk = torch.tensor([float(_HYPER_KINDS[h]) for h in names], dtype=torch.float64)
        hm, his, lin_tau = torch.zeros(G, dtype=torch.float64), torch.zeros(G, dtype=torch.float64), -n_g
        for g, h in enumerate(names):
            if h == "lognormal":
                hm[g], his[g] = loc[g], 1.0 / scl[g]
                c += -math.log(float(scl[g])) - 0.5 * L2PI
            else:  # a density over sigma = exp(tau): + tau_g from the change of variables
                hm[g] = math.log(float(scl[g]))
                lin_tau[g] += 1.0
                c += (0.5 if h == "halfnormal" else 1.0) * math.log(2.0 / math.pi) - float(hm[g])
        order = torch.argsort(grp, stable=True)                                            # members in increasing feature index
        gidx = torch.cat([order[grp[order] >= 0], torch.zeros(int((~grouped).sum()), dtype=torch.int64)]).to(torch.float64)
        gptr = torch.cat([torch.zeros(1, dtype=torch.float64), torch.cumsum(n_g, 0)])
        self.family, self.d, self.p, self.G, self.rows, self.param, self.const = family, d, p, G, rows, param, c
        self.groups, self.hyper = grp, names
        self.A = torch.cat([A.detach(), torch.zeros(rows, G, dtype=A.dtype, device=A.device)], 1).contiguous()
        self.p0 = torch.cat([ln, lin_tau, off, wt, torch.tensor([param, c], dtype=torch.float64), grp.to(torch.float64), isd, hm, his, hk,
                             gptr, gidx]).to(A.dtype).to(A.device).contiguous()
        self.c = Target(_HGLM_KINDS[family], self.p0.data_ptr(), self.A.data_ptr(), float(rows), float(G))

    def coefficients(self, y):
        """beta, the first p leading elements of a parameter vector (d,) or a batch (d, N)"""
        return y[:self.p]

    def scales(self, y):
        """the group scales exp(tau) of a parameter vector (d,) or a batch (d, N)"""
        return torch.exp(y[self.p:])


class VaryingInterceptTarget(HierarchicalGLMTarget):
    """A GLM with one varying (random) intercept per level: u_i = x_i . b + a_{level_of_row[i]} + offset_i, with
    a_l ~ N(0, exp(tau)^2) sharing ONE learned scale and the columns of X under fixed_sigma.  Builds A = [X | one-hot(level)],
    z = [b (X's columns) ; a (n_levels) ; tau]."""

    def __init__(self, family, X, level_of_row, n_levels, offset=None, weights=None, lin=None, const=0.0, param=0.0, fixed_sigma=1.0,
                 hyper="halfcauchy", hyper_loc=0.0, hyper_scale=1.0):
        nm = "VaryingInterceptTarget"
        _glm_matrix(nm, X)
        rows, px = X.shape
        if isinstance(n_levels, bool) or not hasattr(n_levels, "__index__") or int(n_levels) < 1:
            raise NFHipError(f"{nm}: n_levels must be an integer >= 1")
        L = int(n_levels)
        if not isinstance(level_of_row, torch.Tensor) or level_of_row.dim() != 1 or level_of_row.numel() != rows or \
                level_of_row.dtype.is_floating_point or level_of_row.dtype.is_complex or level_of_row.dtype == torch.bool:
            raise NFHipError(f"{nm}: level_of_row must be an integer tensor with one level per row of X")
        lev = level_of_row.detach().to("cpu", torch.int64)
        if bool((lev < 0).any()) or bool((lev >= L).any()):
            raise NFHipError(f"{nm}: levels must be in 0..{L - 1}")
        onehot = torch.zeros(rows, L, dtype=X.dtype)
        onehot[torch.arange(rows), lev] = 1.0
        A = torch.cat([X.detach(), onehot.to(X.device)], 1)
        groups = torch.cat([torch.full((px,), -1, dtype=torch.int64), torch.zeros(L, dtype=torch.int64)])
        if lin is not None and isinstance(lin, torch.Tensor) and lin.dim() == 1 and lin.numel() == px:
            lin = torch.cat([lin, torch.zeros(L, dtype=lin.dtype, device=lin.device)])
        sig = _per_item(nm, "fixed_sigma", fixed_sigma, px, positive=True, allow_inf=True)
        self.n_levels, self.levels = L, lev
        super().__init__(family, A, groups, 1, offset, weights, lin, const, param, torch.cat([sig, torch.ones(L, dtype=torch.float64)]),
                         hyper, hyper_loc, hyper_scale, _name=nm)


_DGLM_KINDS = {"normal": _lib.NF_TARGET_DGLM_NORMAL, "student": _lib.NF_TARGET_DGLM_STUDENT, "negbin": _lib.NF_TARGET_DGLM_NEGBIN}
_DGLM_MAX_COUNT = 4097  # the device's table T(lambda) holds at most 4096 entries c_1 .. c_{max k - 1}


class DispersionGLMTarget(_LinpredTarget):
    """A GLM posterior with a LEARNED dispersion (NF_TARGET_DGLM_*), over z = [beta (p coefficients) ; tau (G group log-scales) ;
    lambda (the log-dispersion)], d = p + G + 1, under HierarchicalGLMTarget's structured prior on (beta, tau):
        logp(z) = const + sum_i weights_i l_i(u_i, lambda) + lin . beta + sum_j log N(beta_j; 0, sigma_j^2) + sum_g log p(tau_g) + log p(lambda),
        u = A beta + offset.
    family "normal":  l_i = -z_i^2 / 2 - lambda,                          z_i = u_i exp(-lambda)   (sigma = exp(lambda); -log(2 pi)/2 is the caller's const)
           "student": l_i = -(nu + 1)/2 log1p(z_i^2 / nu) - lambda,       nu = param
           "negbin":  l_i = log NB(counts_i; mean exp(u_i), size exp(lambda)), the full log-pmf (lgamma(k + 1) included)
    A [rows, p], groups, n_groups, offset, weights, lin (p,), const, param, fixed_sigma, hyper, hyper_loc, hyper_scale are
    HierarchicalGLMTarget's (groups=None: every coefficient under fixed_sigma).  counts: non-negative integers <= 4097, required for
    and only for "negbin".  disp_hyper / disp_loc / disp_scale: the prior of exp(lambda), one of the three hyper-prior forms.
    Everything linear in z or constant is folded here in float64: the -(sum weights) lambda of the scale families' normalisers and the
    Jacobians into lin, the counts' sum_i w_i k_i u_i into lin and the constant, c_m = sum_{i: k_i > m} w_i into the table.  The
    device reads `A` (padded with zero tau- and lambda-columns to [rows, d]) and ONE buffer `p0` (include/nfhip.h)."""

    def __init__(self, family, A, counts=None, groups=None, n_groups=0, offset=None, weights=None, lin=None, const=0.0, param=0.0,
                 fixed_sigma=1.0, hyper="halfcauchy", hyper_loc=0.0, hyper_scale=1.0, disp_hyper="halfcauchy", disp_loc=0.0, disp_scale=1.0,
                 _name="DispersionGLMTarget"):
        nm = _name
        if family not in _DGLM_KINDS:
            raise NFHipError(f"{nm}: family must be one of {sorted(_DGLM_KINDS)}")
        A64 = _glm_matrix(nm, A)
        rows, p = A64.shape
        if isinstance(n_groups, bool) or not hasattr(n_groups, "__index__") or int(n_groups) < 0:
            raise NFHipError(f"{nm}: n_groups must be an integer >= 0")
        G = int(n_groups)
        d = p + G + 1
        if d > 256:
            raise NFHipError(f"{nm}: p + n_groups + 1 = {d} exceeds the kernels' d = 256")
        if groups is None:
            groups = torch.full((p,), -1, dtype=torch.int64)
        if not isinstance(groups, torch.Tensor) or groups.dim() != 1 or groups.numel() != p or groups.dtype.is_floating_point or \
                groups.dtype.is_complex or groups.dtype == torch.bool:
            raise NFHipError(f"{nm}: groups must be an integer tensor of length {p}")
        grp = groups.detach().to("cpu", torch.int64)
        if bool((grp < -1).any()) or bool((grp >= G).any()):
            raise NFHipError(f"{nm}: groups must hold -1 (a fixed prior scale) or a group index in 0..{G - 1}")
        off = _glm_vector(nm, "offset", offset, A, rows, 0.0)
        wt = _glm_vector(nm, "weights", weights, A, rows, 1.0, nonneg=True)
        ln = _glm_vector(nm, "lin", lin, A, p, 0.0)
        const = _glm_scalar(nm, "const", const, positive=False)
        param = _glm_scalar(nm, "param", param, positive=family == "student")
        sig = _per_item(nm, "fixed_sigma", fixed_sigma, p, positive=True, allow_inf=True)
        names = [hyper] * G if isinstance(hyper, str) else list(hyper)
        if len(names) != G or any(not isinstance(h, str) or h not in _HYPER_KINDS for h in names):
            raise NFHipError(f"{nm}: hyper must be one of {sorted(_HYPER_KINDS)}, or one of them per group")
        if not isinstance(disp_hyper, str) or disp_hyper not in _HYPER_KINDS:
            raise NFHipError(f"{nm}: disp_hyper must be one of {sorted(_HYPER_KINDS)}")
        loc = torch.cat([_per_item(nm, "hyper_loc", hyper_loc, G), torch.tensor([_glm_scalar(nm, "disp_loc", disp_loc, positive=False)], dtype=torch.float64)])
        scl = torch.cat([_per_item(nm, "hyper_scale", hyper_scale, G, positive=True), torch.tensor([_glm_scalar(nm, "disp_scale", disp_scale)], dtype=torch.float64)])
        names_all = names + [disp_hyper]
        if (family == "negbin") != (counts is not None):
            raise NFHipError(f"{nm}: counts are required for, and only for, the negbin family")

        grouped = grp >= 0
        isd = torch.where(grouped, torch.zeros(p, dtype=torch.float64), 1.0 / sig)        # 1 / inf = 0: flat
        n_g = torch.bincount(grp[grouped], minlength=G).to(torch.float64) if G else torch.zeros(0, dtype=torch.float64)
        L2PI = math.log(2.0 * math.pi)
        fixed = (~grouped) & torch.isfinite(sig)
        c = const - float(torch.log(sig[fixed]).sum()) - 0.5 * L2PI * float(fixed.sum()) - 0.5 * L2PI * float(grouped.sum())
        hk = torch.tensor([float(_HYPER_KINDS[h]) for h in names_all], dtype=torch.float64)
        hm, his = torch.zeros(G + 1, dtype=torch.float64), torch.zeros(G + 1, dtype=torch.float64)
        lin_tl = torch.cat([-n_g, torch.zeros(1, dtype=torch.float64)])                    # lin of [tau ; lambda]
        for g, h in enumerate(names_all):
            if h == "lognormal":
                hm[g], his[g] = loc[g], 1.0 / scl[g]
                c += -math.log(float(scl[g])) - 0.5 * L2PI
            else:  # a density over exp(.): + tau_g (+ lambda) from the change of variables
                hm[g] = math.log(float(scl[g]))
                lin_tl[g] += 1.0
                c += (0.5 if h == "halfnormal" else 1.0) * math.log(2.0 / math.pi) - float(hm[g])
        tail = []
        mt = 0
        if family == "negbin":
            k = _glm_vector(nm, "counts", counts, A, rows, nonneg=True)
            if bool((k != torch.round(k)).any()) or bool((k > _DGLM_MAX_COUNT).any()):
                raise NFHipError(f"{nm}: counts must be integers in 0..{_DGLM_MAX_COUNT}")
            live = wt > 0                                                                  # zero-weight rows never enter the table
            M = int(k[live].max()) if bool(live.any()) else 0
            mt = max(M - 1, 0)
            m = torch.arange(1, mt + 1, dtype=torch.float64)
            ctab = ((k[None, :] > m[:, None]).to(torch.float64) * wt[None, :]).sum(1)     # c_m = sum_{i: k_i > m} w_i, m = 1 .. M - 1
            kl, wl, ol = k[live], wt[live], off[live]                                      # nor the folded sums: a masked row changes no bit of p0
            ln = ln + (wl * kl) @ A64[live]
            c += float((wl * (kl * ol - torch.lgamma(kl + 1.0))).sum())
            tail = [k, ctab]
            self.counts = k
        else:
            lin_tl[G] -= float(wt[wt > 0].sum())                                           # the -lambda of every live row's normaliser
        order = torch.argsort(grp, stable=True)                                            # members in increasing feature index
        gidx = torch.cat([order[grp[order] >= 0], torch.zeros(int((~grouped).sum()), dtype=torch.int64)]).to(torch.float64)
        gptr = torch.cat([torch.zeros(1, dtype=torch.float64), torch.cumsum(n_g, 0)])
        self.family, self.d, self.p, self.G, self.rows, self.param, self.const = family, d, p, G, rows, param, c
        self.groups, self.hyper, self.disp_hyper, self.table_len = grp, names, disp_hyper, mt
        self.A = torch.cat([A.detach(), torch.zeros(rows, G + 1, dtype=A.dtype, device=A.device)], 1).contiguous()
        self.p0 = torch.cat([ln, lin_tl, off, wt, torch.tensor([param, c, float(mt), 0.0], dtype=torch.float64), grp.to(torch.float64), isd, hm, his,
                             hk, gptr, gidx] + tail).to(A.dtype).to(A.device).contiguous()
        self.c = Target(_DGLM_KINDS[family], self.p0.data_ptr(), self.A.data_ptr(), float(rows), float(G))

    def coefficients(self, y):
        """beta, the first p leading elements of a parameter vector (d,) or a batch (d, N)"""
        return y[:self.p]

    def scales(self, y):
        """the group scales exp(tau) of a parameter vector (d,) or a batch (d, N)"""
        return torch.exp(y[self.p:self.p + self.G])

    def dispersion(self, y):
        """exp(lambda): the residual scale sigma (normal, student) or the negative binomial's size r"""
        return torch.exp(y[-1])


def _residual_rows(nm, X, y, weights):
    X64 = _glm_matrix(nm, X)
    n = X64.shape[0]
    yv = _glm_vector(nm, "y", y, X, n)
    w = _glm_vector(nm, "weights", weights, X, n, 1.0, nonneg=True)
    return yv, w


class GaussianRegressionTarget(DispersionGLMTarget):
    """Posterior of Gaussian linear regression with an UNKNOWN noise scale: y_i ~ N(x_i . b, sigma^2), z = [b ; log sigma], the
    columns of X under N(0, fixed_sigma^2) and sigma under disp_hyper.  Folds to the "normal" family with A = X, offset = -y and
    const = -(sum_i w_i) log(2 pi) / 2."""

    def __init__(self, X, y, weights=None, fixed_sigma=1.0, disp_hyper="halfcauchy", disp_loc=0.0, disp_scale=1.0):
        nm = "GaussianRegressionTarget"
        yv, w = _residual_rows(nm, X, y, weights)
        to = lambda t: t.to(X.dtype).to(X.device)
        super().__init__("normal", X, offset=to(-yv), weights=to(w), const=-0.5 * math.log(2.0 * math.pi) * float(w.sum()), fixed_sigma=fixed_sigma,
                         disp_hyper=disp_hyper, disp_loc=disp_loc, disp_scale=disp_scale, _name=nm)


class StudentRegressionTarget(DispersionGLMTarget):
    """Posterior of linear regression with Student-t noise of an UNKNOWN scale: (y_i - x_i . b) / sigma ~ t_nu, z = [b ; log sigma].
    Folds to the "student" family with A = X, offset = -y, param = nu and
    const = sum_i w_i (lgamma((nu+1)/2) - lgamma(nu/2) - log(nu pi)/2)."""

    def __init__(self, X, y, nu, weights=None, fixed_sigma=1.0, disp_hyper="halfcauchy", disp_loc=0.0, disp_scale=1.0):
        nm = "StudentRegressionTarget"
        yv, w = _residual_rows(nm, X, y, weights)
        nu = _glm_scalar(nm, "nu", nu)
        const = float(w.sum()) * (math.lgamma(0.5 * (nu + 1.0)) - math.lgamma(0.5 * nu) - 0.5 * math.log(nu * math.pi))
        to = lambda t: t.to(X.dtype).to(X.device)
        super().__init__("student", X, offset=to(-yv), weights=to(w), const=const, param=nu, fixed_sigma=fixed_sigma, disp_hyper=disp_hyper,
                         disp_loc=disp_loc, disp_scale=disp_scale, _name=nm)


class NegativeBinomialRegressionTarget(DispersionGLMTarget):
    """Posterior of negative-binomial regression (log link) with an UNKNOWN size: counts k_i ~ NB(mean exposure_i exp(x_i . b),
    size r), z = [b ; log r].  Folds to the "negbin" family with A = X and offset = log exposure."""

    def __init__(self, X, counts, exposure=None, weights=None, fixed_sigma=1.0, disp_hyper="halfcauchy", disp_loc=0.0, disp_scale=1.0):
        nm = "NegativeBinomialRegressionTarget"
        X64 = _glm_matrix(nm, X)
        n = X64.shape[0]
        off = torch.log(_glm_vector(nm, "exposure", exposure, X, n, 1.0, positive=True))
        super().__init__("negbin", X, counts=counts, offset=off.to(X.dtype).to(X.device), weights=weights, fixed_sigma=fixed_sigma,
                         disp_hyper=disp_hyper, disp_loc=disp_loc, disp_scale=disp_scale, _name=nm)


class LinearMixedModelTarget(DispersionGLMTarget):
    """The linear mixed model y ~ x + (1 | level): y_i ~ N(x_i . b + a_{level_of_row[i]}, sigma^2) with a_l ~ N(0, exp(tau)^2) sharing
    ONE learned scale, the columns of X under fixed_sigma and the residual sigma = exp(lambda) learned too.  Builds
    A = [X | one-hot(level)], z = [b (X's columns) ; a (n_levels) ; tau ; lambda]."""

    def __init__(self, X, y, level_of_row, n_levels, weights=None, fixed_sigma=1.0, hyper="halfcauchy", hyper_loc=0.0, hyper_scale=1.0,
                 disp_hyper="halfcauchy", disp_loc=0.0, disp_scale=1.0):
        nm = "LinearMixedModelTarget"
        yv, w = _residual_rows(nm, X, y, weights)
        rows, px = X.shape
        if isinstance(n_levels, bool) or not hasattr(n_levels, "__index__") or int(n_levels) < 1:
            raise NFHipError(f"{nm}: n_levels must be an integer >= 1")
        L = int(n_levels)
        if not isinstance(level_of_row, torch.Tensor) or level_of_row.dim() != 1 or level_of_row.numel() != rows or \
                level_of_row.dtype.is_floating_point or level_of_row.dtype.is_complex or level_of_row.dtype == torch.bool:
            raise NFHipError(f"{nm}: level_of_row must be an integer tensor with one level per row of X")
        lev = level_of_row.detach().to("cpu", torch.int64)
        if bool((lev < 0).any()) or bool((lev >= L).any()):
            raise NFHipError(f"{nm}: levels must be in 0..{L - 1}")
        onehot = torch.zeros(rows, L, dtype=X.dtype)
        onehot[torch.arange(rows), lev] = 1.0
        A = torch.cat([X.detach(), onehot.to(X.device)], 1)
        groups = torch.cat([torch.full((px,), -1, dtype=torch.int64), torch.zeros(L, dtype=torch.int64)])
        sig = _per_item(nm, "fixed_sigma", fixed_sigma, px, positive=True, allow_inf=True)
        self.n_levels, self.levels = L, lev
        to = lambda t: t.to(X.dtype).to(X.device)
        super().__init__("normal", A, groups=groups, n_groups=1, offset=to(-yv), weights=to(w), const=-0.5 * math.log(2.0 * math.pi) * float(w.sum()),
                         fixed_sigma=torch.cat([sig, torch.ones(L, dtype=torch.float64)]), hyper=hyper, hyper_loc=hyper_loc, hyper_scale=hyper_scale,
                         disp_hyper=disp_hyper, disp_loc=disp_loc, disp_scale=disp_scale, _name=nm)


class SoftmaxRegressionTarget(_LinpredTarget):
    """Posterior of Bayesian softmax (multinomial-logit) regression over the weight matrix W [p, C]: data rows X [rows, p],
    labels c_i in {0 .. C-1}, row weights w_i >= 0 (0 drops the row exactly), prior N(0, prior_sigma^2 I):
        logp(z) = const + sum_i w_i (x_i . W[:, c_i] - logsumexp_c x_i . W[:, c]) - |z|^2 / (2 prior_sigma^2) - d/2 log(2 pi prior_sigma^2)
    with z = vec(W) in column-major order (class-major: z = [W[:, 0]; ...; W[:, C-1]], d = C p) -- `weights(z)` gives W back.
    An intercept is a ones column of X.  prior_sigma = math.inf is the flat prior.  The constants are folded in float64; the
    device reads `A` = X and ONE buffer `p0` = labels | weights | (1 / prior_sigma^2, const - d/2 log(2 pi prior_sigma^2)),
    both kept alive here."""

    def __init__(self, X, labels, n_classes=None, weights=None, prior_sigma=1.0, const=0.0, _name="SoftmaxRegressionTarget"):
        nm = _name
        _glm_matrix(nm, X)
        rows, p = X.shape
        lab = _glm_vector(nm, "labels", labels, X, rows)
        if bool((lab != torch.round(lab)).any()) or bool((lab < 0).any()):
            raise NFHipError(f"{nm}: labels must be integers >= 0")
        C_ = int(lab.max()) + 1 if n_classes is None else n_classes
        if isinstance(C_, float) and C_ == int(C_):
            C_ = int(C_)
        if isinstance(C_, bool) or not hasattr(C_, "__index__") or not 2 <= int(C_) <= 16:
            raise NFHipError(f"{nm}: the number of classes must be an integer in 2..16" + (" (give n_classes)" if n_classes is None else ""))
        C_ = int(C_)
        if bool((lab >= C_).any()):
            raise NFHipError(f"{nm}: labels must be in 0..{C_ - 1}")
        if C_ * p > 256:
            raise NFHipError(f"{nm}: n_classes * p = {C_ * p} exceeds the kernels' d = 256")
        wt = _glm_vector(nm, "weights", weights, X, rows, 1.0, nonneg=True)
        const = _glm_scalar(nm, "const", const, positive=False)
        self.prior_sigma = _glm_scalar(nm, "prior_sigma", prior_sigma, allow_inf=True)
        d = C_ * p
        flat = math.isinf(self.prior_sigma)
        self.precision = 0.0 if flat else 1.0 / self.prior_sigma**2
        self.const = const + (0.0 if flat else -0.5 * d * math.log(2.0 * math.pi * self.prior_sigma**2))
        self.d, self.p, self.n_classes, self.rows = d, p, C_, rows
        self.A = X.detach().contiguous()
        self.X = self.A
        self.p0 = torch.cat([lab, wt, torch.tensor([self.precision, self.const], dtype=torch.float64)]).to(X.dtype).to(X.device).contiguous()
        self.c = Target(_lib.NF_TARGET_SOFTMAX, self.p0.data_ptr(), self.A.data_ptr(), float(rows), float(C_))

    def weights(self, y):
        """the weight matrix W [p, C] of a parameter vector y (d,) -- or [p, C, N] of a batch (d, N)"""
        if y.shape[0] != self.d:
            raise NFHipError(f"SoftmaxRegressionTarget.weights: expected {self.d} leading elements, got {y.shape[0]}")
        W = y.reshape(self.n_classes, self.p, *y.shape[1:])
        return W.transpose(0, 1)


class MultinomialRegressionTarget(SoftmaxRegressionTarget):
    """Posterior of multinomial (softmax-link) regression on count data: counts[i, :] ~ Multinomial(n_i, softmax(x_i W)),
    n_i = sum_c counts[i, c].  Expands to one softmax row per non-zero (i, c) with weight counts[i, c] * weights[i] and folds
    sum_i weights_i [lgamma(n_i + 1) - sum_c lgamma(counts[i, c] + 1)] into the constant."""

    def __init__(self, X, counts, weights=None, prior_sigma=1.0):
        nm = "MultinomialRegressionTarget"
        _glm_matrix(nm, X)
        n = X.shape[0]
        if not isinstance(counts, torch.Tensor) or counts.dim() != 2 or counts.shape[0] != n or counts.device != X.device or \
                (counts.dtype.is_floating_point and counts.dtype != X.dtype) or counts.dtype.is_complex or counts.dtype == torch.bool:
            raise NFHipError(f"{nm}: counts must be a matrix [rows, C] on the data matrix's device, of its element type or an integer tensor")
        C_ = counts.shape[1]
        if not 2 <= C_ <= 16:
            raise NFHipError(f"{nm}: the number of classes (columns of counts) must be in 2..16")
        k = counts.detach().to("cpu", torch.float64)
        if not bool(torch.isfinite(k).all()) or bool((k < 0).any()) or bool((k != torch.round(k)).any()):
            raise NFHipError(f"{nm}: counts must be non-negative integers")
        w = _glm_vector(nm, "weights", weights, X, n, 1.0, nonneg=True)
        i_idx, c_idx = torch.nonzero(k, as_tuple=True)
        if i_idx.numel() == 0:
            raise NFHipError(f"{nm}: every count is zero")
        coef = torch.lgamma(k.sum(1) + 1.0) - torch.lgamma(k + 1.0).sum(1)
        const = float((w * coef).sum())
        to = lambda t: t.to(X.dtype).to(X.device)
        self.counts = k
        super().__init__(X.detach()[i_idx.to(X.device)], to(c_idx.to(torch.float64)), C_, to(k[i_idx, c_idx] * w[i_idx]), prior_sigma, const, _name=nm)


_BNN_KINDS = {"logit": _lib.NF_TARGET_BNN_LOGIT, "probit": _lib.NF_TARGET_BNN_PROBIT, "poisson": _lib.NF_TARGET_BNN_POISSON,
              "student": _lib.NF_TARGET_BNN_STUDENT, "normal": _lib.NF_TARGET_BNN_NORMAL}


class BNNTarget(_LinpredTarget):
    """Posterior of a one-hidden-layer Bayesian neural network (NF_TARGET_BNN_*) over its weights, z = [w_0; ...; w_{H-1}; v; c]
    (hidden-unit-major: w_k the p input weights of unit k, v the H output weights, c the output bias; d = H (p + 1) + 1):
        a_ik = tanh(x_i . w_k),   f_i = c + sum_k v_k a_ik,   u_i = scale_i f_i + offset_i,
        logp(z) = const + sum_i weights_i phi(u_i; param) + sum_k log N(w_k; 0, prior_sigma_hidden^2 I) + log N([v; c]; 0, prior_sigma_out^2 I)
    family and phi are GLMTarget's.  X [rows, p] (a hidden bias is a ones column); scale, offset, weights (>= 0; 0 drops the row
    exactly) per row, of X's element type and device.  scale and offset carry the likelihood: labels +-1 in scale for "logit" /
    "probit", scale = 1 / sigma and offset = -t / sigma for Gaussian or Student noise, log-exposures in offset for "poisson".
    prior_sigma_* = math.inf is the flat prior.  Both Gaussian normalisers and const are folded in float64; the device reads
    `A` = X and ONE buffer `p0` = scale | offset | weights | (param, const, 1 / prior_sigma_hidden^2, 1 / prior_sigma_out^2),
    both kept alive here."""

    def __init__(self, family, X, n_hidden, scale=None, offset=None, weights=None, const=0.0, param=None, prior_sigma_hidden=1.0,
                 prior_sigma_out=1.0, _name="BNNTarget"):
        nm = _name
        if family not in _BNN_KINDS:
            raise NFHipError(f"{nm}: family must be one of {sorted(_BNN_KINDS)}")
        _glm_matrix(nm, X)
        rows, p = X.shape
        H = n_hidden
        if isinstance(H, float) and H == int(H):
            H = int(H)
        if isinstance(H, bool) or not hasattr(H, "__index__") or not 1 <= int(H) <= 16:
            raise NFHipError(f"{nm}: n_hidden must be an integer in 1..16")
        H = int(H)
        if p > 128:
            raise NFHipError(f"{nm}: p = {p} input features exceed the kernels' 128")
        d = H * (p + 1) + 1
        if d > 256:
            raise NFHipError(f"{nm}: n_hidden * (p + 1) + 1 = {d} exceeds the kernels' d = 256")
        scl = _glm_vector(nm, "scale", scale, X, rows, 1.0)
        off = _glm_vector(nm, "offset", offset, X, rows, 0.0)
        wt = _glm_vector(nm, "weights", weights, X, rows, 1.0, nonneg=True)
        const = _glm_scalar(nm, "const", const, positive=False)
        if param is None:
            if family == "student":
                raise NFHipError(f"{nm}: the student family needs param = nu > 0")
            param = 0.0
        param = _glm_scalar(nm, "param", param, positive=family == "student")
        self.prior_sigma_hidden = _glm_scalar(nm, "prior_sigma_hidden", prior_sigma_hidden, allow_inf=True)
        self.prior_sigma_out = _glm_scalar(nm, "prior_sigma_out", prior_sigma_out, allow_inf=True)
        c = const
        prec = []
        for sigma, count in ((self.prior_sigma_hidden, H * p), (self.prior_sigma_out, H + 1)):
            flat = math.isinf(sigma)
            prec.append(0.0 if flat else 1.0 / sigma**2)
            c += 0.0 if flat else -0.5 * count * math.log(2.0 * math.pi * sigma**2)
        self.family, self.d, self.p, self.n_hidden, self.rows, self.param, self.const = family, d, p, H, rows, param, c
        self.precision_hidden, self.precision_out = prec
        self.A = X.detach().contiguous()
        self.X = self.A
        self.p0 = torch.cat([scl, off, wt, torch.tensor([param, c, prec[0], prec[1]], dtype=torch.float64)]).to(X.dtype).to(X.device).contiguous()
        self.c = Target(_BNN_KINDS[family], self.p0.data_ptr(), self.A.data_ptr(), float(rows), float(H))

    def unpack(self, y):
        """(W [p, H], v [H], c) of a parameter vector y (d,) -- or (W [p, H, N], v [H, N], c [N]) of a batch (d, N)"""
        if y.shape[0] != self.d:
            raise NFHipError(f"BNNTarget.unpack: expected {self.d} leading elements, got {y.shape[0]}")
        H, p = self.n_hidden, self.p
        W = y[:H * p].reshape(H, p, *y.shape[1:]).transpose(0, 1)
        return W, y[H * p:H * p + H], y[self.d - 1]

    def predict(self, y, Xnew):
        """the network's output f = c + tanh(Xnew W) v in plain torch: [rows] for a vector y, [rows, N] for a batch (d, N)"""
        if Xnew.dim() != 2 or Xnew.shape[1] != self.p:
            raise NFHipError(f"BNNTarget.predict: Xnew must be a matrix [rows, {self.p}]")
        W, v, c = self.unpack(y)
        if y.dim() == 1:
            return torch.tanh(Xnew @ W) @ v + c
        return torch.einsum("ikn,kn->in", torch.tanh(torch.einsum("if,fkn->ikn", Xnew, W)), v) + c.unsqueeze(0)


class BNNRegressionTarget(BNNTarget):
    """Posterior of a one-hidden-layer network regressing t on X: t_i ~ N(f_i, noise_sigma^2), or (t_i - f_i) / noise_sigma ~ t_nu
    when `nu` is given.  Folds to the "normal" / "student" family with scale = 1 / noise_sigma, offset = -t / noise_sigma and the
    noise normaliser sum_i w_i (...) in the constant."""

    def __init__(self, X, t, n_hidden, noise_sigma=1.0, nu=None, weights=None, prior_sigma_hidden=1.0, prior_sigma_out=1.0):
        nm = "BNNRegressionTarget"
        _glm_matrix(nm, X)
        n = X.shape[0]
        tv = _glm_vector(nm, "t", t, X, n)
        sn = _glm_scalar(nm, "noise_sigma", noise_sigma)
        w = _glm_vector(nm, "weights", weights, X, n, 1.0, nonneg=True)
        if nu is None:
            family, param = "normal", None
            const = float(w.sum()) * (-0.5 * math.log(2.0 * math.pi) - math.log(sn))
        else:
            family, param = "student", _glm_scalar(nm, "nu", nu)
            const = float(w.sum()) * (math.lgamma(0.5 * (param + 1.0)) - math.lgamma(0.5 * param) - 0.5 * math.log(param * math.pi) - math.log(sn))
        to = lambda x: x.to(X.dtype).to(X.device)
        # f - t enters squared (or through u^2): scale = -1 / sigma would do as well; +1 / sigma keeps u = (f - t) / sigma
        super().__init__(family, X, n_hidden, to(torch.full((n,), 1.0 / sn, dtype=torch.float64)), to(-tv / sn), to(w), const, param,
                         prior_sigma_hidden, prior_sigma_out, _name=nm)


class BNNClassifierTarget(BNNTarget):
    """Posterior of a one-hidden-layer binary classifier: P(label_i = 1) = sigmoid(f_i) (link="logit") or Phi(f_i) ("probit"),
    labels in {0, 1}.  The labels are folded into the rows' scale (+-1)."""

    def __init__(self, X, labels, n_hidden, link="logit", weights=None, prior_sigma_hidden=1.0, prior_sigma_out=1.0):
        nm = "BNNClassifierTarget"
        if link not in ("logit", "probit"):
            raise NFHipError(f"{nm}: link must be \"logit\" or \"probit\"")
        _glm_matrix(nm, X)
        n = X.shape[0]
        lab = _glm_vector(nm, "labels", labels, X, n)
        if not bool(((lab == 0) | (lab == 1)).all()):
            raise NFHipError(f"{nm}: labels must be in {{0, 1}}")
        w = _glm_vector(nm, "weights", weights, X, n, 1.0, nonneg=True)
        to = lambda x: x.to(X.dtype).to(X.device)
        super().__init__(link, X, n_hidden, to(2.0 * lab - 1.0), None, to(w), 0.0, None, prior_sigma_hidden, prior_sigma_out, _name=nm)


class OrdinalRegressionTarget(_LinpredTarget):
    """Posterior of ordinal (cumulative-logit, proportional-odds) regression (NF_TARGET_ORDINAL_LOGIT): labels k_i in {0 .. C-1},
    one linear predictor eta_i = x_i . beta + offset_i per row and C - 1 ordered cutpoints that are coordinates:
        z = [beta (p) ; gamma (C - 1)],  d = p + C - 1;   c_1 = gamma_1,  c_k = c_{k-1} + exp(gamma_k),
        P(k_i) = sigmoid(c_{k_i + 1} - eta_i) - sigmoid(c_{k_i} - eta_i)   (c_0 = -inf, c_C = +inf),
        logp(z) = const + sum_i weights_i log P(k_i) + log N(beta; 0, prior_sigma^2 I) + sum_k log N(c_k; cut_loc, cut_sigma^2)
                  + sum_{k>=2} gamma_k
    -- a density over the unconstrained z (the last sum is the ordered transform's Jacobian).  X [rows, p] has NO intercept
    column (the cutpoints are the intercepts); offset, weights (>= 0; 0 drops the row exactly) per row, of X's element type and
    device.  prior_sigma = math.inf and cut_sigma = math.inf are the flat priors.  The host works in float64: it sorts the rows by
    label (stably), pads every label to whole 32-row blocks with rows of weight 0 (a category without rows gets no block), folds
    n_k = sum_i weights_i [k_i = k], both Gaussian normalisers and const; the device reads `A` = the padded X [R, p] and ONE buffer
    `p0` = offset[R] | weights[R] | block labels[R / 32] | (1 / prior_sigma^2, const, 1 / cut_sigma^2, cut_loc) | n_k[C], both
    kept alive here.  `rows` is the caller's row count, `padded_rows` is R."""

    def __init__(self, X, labels, n_categories, offset=None, weights=None, prior_sigma=1.0, cut_sigma=1.0, cut_loc=0.0, const=0.0,
                 _name="OrdinalRegressionTarget"):
        nm = _name
        X64 = _glm_matrix(nm, X)
        rows, p = X.shape
        C_ = n_categories
        if isinstance(C_, float) and C_ == int(C_):
            C_ = int(C_)
        if isinstance(C_, bool) or not hasattr(C_, "__index__") or not 2 <= int(C_) <= 16:
            raise NFHipError(f"{nm}: n_categories must be an integer in 2..16")
        C_ = int(C_)
        d = p + C_ - 1
        if d > 256:
            raise NFHipError(f"{nm}: p + n_categories - 1 = {d} exceeds the kernels' d = 256")
        lab = _glm_vector(nm, "labels", labels, X, rows)
        if bool((lab != torch.round(lab)).any()) or bool((lab < 0).any()) or bool((lab >= C_).any()):
            raise NFHipError(f"{nm}: labels must be integers in 0..{C_ - 1}")
        off = _glm_vector(nm, "offset", offset, X, rows, 0.0)
        wt = _glm_vector(nm, "weights", weights, X, rows, 1.0, nonneg=True)
        const = _glm_scalar(nm, "const", const, positive=False)
        self.prior_sigma = _glm_scalar(nm, "prior_sigma", prior_sigma, allow_inf=True)
        self.cut_sigma = _glm_scalar(nm, "cut_sigma", cut_sigma, allow_inf=True)
        self.cut_loc = _glm_scalar(nm, "cut_loc", cut_loc, positive=False)
        c = const
        prec = []
        for sigma, count in ((self.prior_sigma, p), (self.cut_sigma, C_ - 1)):
            flat = math.isinf(sigma)
            prec.append(0.0 if flat else 1.0 / sigma**2)
            c += 0.0 if flat else -0.5 * count * math.log(2.0 * math.pi * sigma**2)
        lab_i = lab.to(torch.int64)
        order = torch.argsort(lab_i, stable=True)
        counts = torch.bincount(lab_i, minlength=C_)
        nblk = (counts + 31) // 32
        R = int(nblk.sum()) * 32
        Xp = torch.zeros((R, p), dtype=torch.float64)
        offp, wtp = torch.zeros(R, dtype=torch.float64), torch.zeros(R, dtype=torch.float64)
        start = torch.cumsum(nblk, 0) * 32 - nblk * 32                     # the first padded row of each label
        first = torch.cumsum(counts, 0) - counts                           # the first sorted row of each label
        ls = lab_i[order]
        dest = start[ls] + (torch.arange(rows) - first[ls])
        Xp[dest], offp[dest], wtp[dest] = X64[order], off[order], wt[order]
        blab = torch.repeat_interleave(torch.arange(C_), nblk).to(torch.float64)
        nk = torch.zeros(C_, dtype=torch.float64).index_add_(0, lab_i, wt)
        self.d, self.p, self.n_categories, self.C, self.rows, self.padded_rows, self.const = d, p, C_, C_, rows, R, c
        self.precision, self.cut_precision = prec
        self.order, self.row_index = order, dest                           # padded row dest[i] is the caller's row order[i]
        self.A = Xp.to(X.dtype).to(X.device).contiguous()
        self.X = self.A
        self.p0 = torch.cat([offp, wtp, blab, torch.tensor([prec[0], c, prec[1], self.cut_loc], dtype=torch.float64), nk]).to(X.dtype).to(X.device).contiguous()
        self.c = Target(_lib.NF_TARGET_ORDINAL_LOGIT, self.p0.data_ptr(), self.A.data_ptr(), float(R), float(C_))

    def unpack(self, y):
        """(beta [p], cutpoints [C - 1]) of a parameter vector y (d,) -- or ([p, N], [C - 1, N]) of a batch (d, N); the cutpoints are
        the ordered c_k, not gamma"""
        if y.shape[0] != self.d:
            raise NFHipError(f"OrdinalRegressionTarget.unpack: expected {self.d} leading elements, got {y.shape[0]}")
        gam = y[self.p:]
        return y[:self.p], torch.cumsum(torch.cat([gam[:1], torch.exp(gam[1:])]), 0)

    def predict(self, y, Xnew, offset=None):
        """category probabilities in plain torch: [C, rows] for a vector y, [C, rows, N] for a batch (d, N)"""
        if Xnew.dim() != 2 or Xnew.shape[1] != self.p:
            raise NFHipError(f"OrdinalRegressionTarget.predict: Xnew must be a matrix [rows, {self.p}]")
        beta, cut = self.unpack(y)
        eta = Xnew @ beta                                                   # [rows] or [rows, N]
        if offset is not None:
            eta = eta + (offset if y.dim() == 1 else offset.unsqueeze(1))
        cdf = torch.sigmoid(cut.unsqueeze(1) - eta.unsqueeze(0))            # [C - 1, rows(, N)]
        one, zero = torch.ones_like(cdf[:1]), torch.zeros_like(cdf[:1])
        return torch.cat([cdf, one]) - torch.cat([zero, cdf])


def _rs_vector(name, what, v, n, default=None):
    """a per-row vector as float64 numpy on the host: a tensor, an array or a sequence of length n (None: the default)"""
    if v is None:
        return np.full(n, float(default))
    a = v.detach().to("cpu").numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
    if a.ndim != 1 or a.shape[0] != n or a.dtype.kind not in "biuf":
        raise NFHipError(f"{name}: {what} must be a real vector of length {n}")
    return a.astype(np.float64)


class RiskSetTarget(_LinpredTarget):
    """Posterior of a risk-set regression (NF_TARGET_RISKSET) -- the partial likelihood shared by Cox proportional hazards,
    conditional logit and Plackett-Luce rankings -- over the coefficients z in R^p, the rows ALREADY ordered so that every risk set
    is a prefix of its segment (stratum, choice set):
        eta_i = x_i . z + offset_i,   c_i = log sum_{j in seg(i), j <= i} risk_weight_j exp(eta_j),
        logp(z) = const + lin . z - sum_i event_mass_i c_i + log N(z; 0, prior_sigma^2 I)
    X [rows, p] (Float32 or Float64); segment_start (true where a segment begins; row 0 always does), event_mass (>= 0),
    risk_weight (>= 0, default 1; 0 drops the row from every risk set exactly), offset per row, lin per feature -- tensors, arrays
    or sequences.  prior_sigma = math.inf (the default) is the flat prior.  The host works in float64: it pads the tail to a whole
    32-row block with rows of weight 0 (at most 31; segments are never padded), takes log risk_weight (-inf: dropped), folds the
    prior's normaliser into const; the device reads `A` = the padded X [R, p] and ONE buffer
    `p0` = offset[R] | log risk_weight[R] | event_mass[R] | segment_start[R] | lin[p] | (1 / prior_sigma^2, const), both kept alive
    here.  ValueError for a negative mass or weight, a non-finite input on a live row, or an event mass on a row whose
    positive-weight prefix is empty (its c would be log 0).  `rows` is the caller's row count, `padded_rows` is R."""

    def __init__(self, X, segment_start, event_mass, risk_weight=None, offset=None, lin=None, const=0.0, prior_sigma=math.inf,
                 _name="RiskSetTarget"):
        nm = _name
        if not isinstance(X, torch.Tensor) or X.dim() != 2 or X.shape[0] < 1 or X.shape[1] < 1 or X.dtype not in (torch.float32, torch.float64):
            raise NFHipError(f"{nm}: the data matrix must be a Float32 or Float64 tensor [rows, p] with rows >= 1 and p >= 1")
        rows, p = X.shape
        if p > 256:
            raise NFHipError(f"{nm}: p = {p} exceeds the kernels' d = 256")
        R = (rows + 31) // 32 * 32
        if R > _lib.NF_RISKSET_MAXR:
            raise NFHipError(f"{nm}: {rows} rows exceed the kernels' {_lib.NF_RISKSET_MAXR}")
        X64 = X.detach().to("cpu", torch.float64).numpy()
        seg = _rs_vector(nm, "segment_start", segment_start, rows) != 0
        m = _rs_vector(nm, "event_mass", event_mass, rows)
        w = _rs_vector(nm, "risk_weight", risk_weight, rows, 1.0)
        off = _rs_vector(nm, "offset", offset, rows, 0.0)
        ln = _rs_vector(nm, "lin", lin, p, 0.0)
        const = _glm_scalar(nm, "const", const, positive=False)
        self.prior_sigma = _glm_scalar(nm, "prior_sigma", prior_sigma, allow_inf=True)
        if not np.isfinite(w).all() or not np.isfinite(m).all() or (w < 0).any() or (m < 0).any():
            raise ValueError(f"{nm}: event_mass and risk_weight must be finite and >= 0")
        live = w > 0
        if not np.isfinite(X64[live]).all() or not np.isfinite(off[live]).all() or not np.isfinite(ln).all():
            raise ValueError(f"{nm}: X and offset must be finite on every row of positive risk weight, lin everywhere")
        seg[0] = True
        sid = np.cumsum(seg) - 1                                            # the segment of every row
        first_live = np.full(sid[-1] + 1, rows)
        np.minimum.at(first_live, sid[live], np.nonzero(live)[0])          # the first row of positive weight in every segment
        if ((m > 0) & (np.arange(rows) < first_live[sid])).any():
            raise ValueError(f"{nm}: an event mass sits on a row whose risk set is empty (no row of positive weight before it in its segment)")
        flat = math.isinf(self.prior_sigma)
        prec = 0.0 if flat else 1.0 / self.prior_sigma**2
        c = const + (0.0 if flat else -0.5 * p * math.log(2.0 * math.pi * self.prior_sigma**2))
        Xp = np.zeros((R, p))
        Xp[:rows] = np.where(live[:, None], X64, np.where(np.isfinite(X64), X64, 0.0))  # (a dropped row's non-finite features: 0)
        offp, lwp, mp, sp = np.zeros(R), np.full(R, -np.inf), np.zeros(R), np.zeros(R)
        offp[:rows] = np.where(live | np.isfinite(off), off, 0.0)
        with np.errstate(divide="ignore"):
            lwp[:rows] = np.log(w)
        mp[:rows], sp[:rows] = m, seg
        self.d, self.p, self.rows, self.padded_rows, self.const, self.precision = p, p, rows, R, c, prec
        self.segment_start, self.segment_index = torch.from_numpy(seg.copy()), torch.from_numpy(sid)
        self.A = torch.from_numpy(Xp).to(X.dtype).to(X.device).contiguous()
        self.X = self.A
        self.p0 = torch.from_numpy(np.concatenate([offp, lwp, mp, sp, ln, [prec, c]])).to(X.dtype).to(X.device).contiguous()
        self.c = Target(_lib.NF_TARGET_RISKSET, self.p0.data_ptr(), self.A.data_ptr(), float(R), self.prior_sigma)

    def unpack(self, y):
        """the coefficients beta of a parameter vector y (p,) -- or [p, N] of a batch; every coordinate is one"""
        if y.shape[0] != self.d:
            raise NFHipError(f"{type(self).__name__}.unpack: expected {self.d} leading elements, got {y.shape[0]}")
        return y


def _rs_like(X, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(X.dtype).to(X.device)


class CoxRegressionTarget(RiskSetTarget):
    """Posterior of Cox proportional-hazards regression under the Breslow partial likelihood: X [rows, p], time and event (0 / 1)
    per row, optional strata (integer labels), case weights and offset.  The host sorts by stratum, then by time DESCENDING with
    equal times contiguous, so that the risk set of a time is a prefix of its stratum; the whole mass sum_i weights_i event_i of a
    time group sits on the group's last row (rows censored at that time are inside the group: they are at risk), risk_weight =
    weights, lin = sum_i weights_i event_i x_i and const takes sum_i weights_i event_i offset_i.  `order` is the sorting permutation
    (sorted row k is the caller's row order[k]).  ties="efron" is not built."""

    def __init__(self, X, time, event, strata=None, weights=None, offset=None, prior_sigma=math.inf, ties="breslow"):
        nm = "CoxRegressionTarget"
        if ties != "breslow":
            raise NotImplementedError(f"{nm}: ties={ties!r} is not built (only 'breslow')")
        if not isinstance(X, torch.Tensor) or X.dim() != 2 or X.shape[0] < 1:
            raise NFHipError(f"{nm}: the data matrix must be a tensor [rows, p]")
        rows = X.shape[0]
        X64 = X.detach().to("cpu", torch.float64).numpy()
        t = _rs_vector(nm, "time", time, rows)
        ev = _rs_vector(nm, "event", event, rows)
        st = _rs_vector(nm, "strata", strata, rows, 0.0)
        wt = _rs_vector(nm, "weights", weights, rows, 1.0)
        off = _rs_vector(nm, "offset", offset, rows, 0.0)
        if not np.isfinite(t).all() or not np.isfinite(st).all() or not ((ev == 0) | (ev == 1)).all():
            raise ValueError(f"{nm}: time and strata must be finite, event 0 or 1")
        if not np.isfinite(wt).all() or (wt < 0).any():
            raise ValueError(f"{nm}: weights must be finite and >= 0")
        order = np.lexsort((-t, st))                                        # stable: by stratum, then by time descending
        ts, ss, es, ws = t[order], st[order], ev[order], wt[order]
        seg = np.r_[True, ss[1:] != ss[:-1]]
        last = np.r_[(ts[1:] != ts[:-1]) | seg[1:], True]                   # the last row of every (stratum, time) group
        gid = np.cumsum(np.r_[0, last[:-1]])
        mass = np.zeros(rows)
        mass[last] = np.bincount(gid, ws * es)
        we = wt * ev
        live = we > 0
        lin = we[live] @ X64[live]
        const = float((we[live] * off[live]).sum())
        self.order = torch.from_numpy(order.copy())
        self.ties = ties
        super().__init__(X[self.order.to(X.device)], seg, mass, ws, off[order], lin, const, prior_sigma, _name=nm)

    def predict(self, y, Xnew):
        """relative hazards exp(Xnew beta) in plain torch: [rows] for a vector y, [rows, N] for a batch (p, N)"""
        if Xnew.dim() != 2 or Xnew.shape[1] != self.p:
            raise NFHipError(f"CoxRegressionTarget.predict: Xnew must be a matrix [rows, {self.p}]")
        return torch.exp(Xnew @ self.unpack(y))


class ConditionalLogitTarget(RiskSetTarget):
    """Posterior of conditional (McFadden) logit: every choice set (matched set, choice occasion) is one segment, exactly one of
    its rows is chosen, P(chosen) = exp(eta_chosen) / sum_{j in set} exp(eta_j).  X [rows, p], choice_set (integer labels), chosen
    (0 / 1) per row; weights per row, constant inside a set (the set's weight).  The host sorts by choice set (stably); risk_weight
    = 1, the set's weight sits on its last row, lin = sum_sets weight x_chosen.  `order` is the sorting permutation."""

    def __init__(self, X, choice_set, chosen, weights=None, prior_sigma=math.inf):
        nm = "ConditionalLogitTarget"
        if not isinstance(X, torch.Tensor) or X.dim() != 2 or X.shape[0] < 1:
            raise NFHipError(f"{nm}: the data matrix must be a tensor [rows, p]")
        rows = X.shape[0]
        X64 = X.detach().to("cpu", torch.float64).numpy()
        cs = _rs_vector(nm, "choice_set", choice_set, rows)
        ch = _rs_vector(nm, "chosen", chosen, rows)
        wt = _rs_vector(nm, "weights", weights, rows, 1.0)
        if not np.isfinite(cs).all() or not ((ch == 0) | (ch == 1)).all() or not np.isfinite(wt).all() or (wt < 0).any():
            raise ValueError(f"{nm}: choice_set must be finite, chosen 0 or 1, weights finite and >= 0")
        order = np.argsort(cs, kind="stable")
        ss, hs, ws = cs[order], ch[order], wt[order]
        seg = np.r_[True, ss[1:] != ss[:-1]]
        sid = np.cumsum(seg) - 1
        if (np.bincount(sid, hs) != 1).any():
            raise ValueError(f"{nm}: every choice set must have exactly one chosen row")
        first = np.nonzero(seg)[0]
        if (ws != ws[first][sid]).any():
            raise ValueError(f"{nm}: weights must be constant inside a choice set")
        last = np.r_[seg[1:], True]
        mass = np.where(last, ws, 0.0)
        pick = (ch == 1) & (wt > 0)
        lin = wt[pick] @ X64[pick]
        self.order = torch.from_numpy(order.copy())
        super().__init__(X[self.order.to(X.device)], seg, mass, None, None, lin, 0.0, prior_sigma, _name=nm)

    def predict(self, y, Xnew, choice_set_new):
        """the within-set choice probabilities in plain torch, in Xnew's row order: [rows] for a vector y, [rows, N] for a batch"""
        if Xnew.dim() != 2 or Xnew.shape[1] != self.p:
            raise NFHipError(f"ConditionalLogitTarget.predict: Xnew must be a matrix [rows, {self.p}]")
        cs = _rs_vector("ConditionalLogitTarget.predict", "choice_set_new", choice_set_new, Xnew.shape[0])
        idx = torch.from_numpy(np.unique(cs, return_inverse=True)[1].reshape(-1)).to(Xnew.device)
        eta = Xnew @ self.unpack(y)
        top = torch.zeros((int(idx.max()) + 1,) + tuple(eta.shape[1:]), dtype=eta.dtype, device=eta.device)
        top = top.scatter_reduce(0, idx.reshape((-1,) + (1,) * (eta.dim() - 1)).expand_as(eta), eta, "amax", include_self=False)
        e = torch.exp(eta - top[idx])
        return e / torch.zeros_like(top).index_add_(0, idx, e)[idx]


def minibatch_segments(target):
    """The layout nf_target_minibatch gathers, for a target it serves: (segments, weight_segment, w) -- the segments of `target.p0`
    in order as (per_row, length) pairs (a per-row segment has length target.rows), the position of the weight segment among them,
    and the row width w of `target.A`.  NFHipError for every other target class."""
    R = getattr(target, "rows", None)
    row, fx = (True, R), lambda n: (False, int(n))
    if isinstance(target, GLMTarget):                   # lin | off | wt | par[2]
        return [fx(target.d), row, row, fx(2)], 2, target.d
    if isinstance(target, HierarchicalGLMTarget):       # lin | off | wt | par[2] | grp | isd | hm | his | hk | gptr | gidx
        p, G = target.p, target.G
        return [fx(target.d), row, row, fx(2), fx(p), fx(p), fx(G), fx(G), fx(G), fx(G + 1), fx(p)], 2, target.d
    if isinstance(target, DispersionGLMTarget):         # lin | off | wt | par[4] | grp | isd | hm | his | hk | gptr | gidx ( | cnt | ctab)
        p, G = target.p, target.G
        tail = [row, fx(target.table_len)] if target.family == "negbin" else []
        return [fx(target.d), row, row, fx(4), fx(p), fx(p), fx(G + 1), fx(G + 1), fx(G + 1), fx(G + 1), fx(p)] + tail, 2, target.d
    if isinstance(target, SoftmaxRegressionTarget):     # lab | wt | par[2]
        return [row, row, fx(2)], 1, target.p
    if isinstance(target, BNNTarget):                   # scl | off | wt | par[4]
        return [row, row, row, fx(4)], 2, target.p
    raise NFHipError(f"MinibatchTarget: {type(target).__name__} has no row-minibatch form: it needs a per-row weight and exchangeable rows "
                     "(GLMTarget, HierarchicalGLMTarget, DispersionGLMTarget, SoftmaxRegressionTarget, BNNTarget and their subclasses; "
                     "logistic regression: GLMTarget('logit', ...) or BinomialRegressionTarget)")


class MinibatchTarget(_LinpredTarget):
    """A row minibatch of a regression target for stochastic VI over many rows: `batch_rows` of `target`'s rows, drawn on the device
    by nf_target_minibatch -- stratified, one row per stratum, without replacement, the weight of row idx_j scaled by the size n_j of
    its stratum -- into buffers of the full target's own kind and layout.  The sum over the batch is an unbiased estimate of the sum
    over all rows; everything the constructor of `target` folded over the full data (lin, the constants, the negative-binomial
    table) is copied and stays exact.  batch_rows == target.rows is the full target bit for bit.
    `.c` describes the CURRENT batch (`.A` [batch_rows, w], `.p0`, `.indices`), `.d` is the full target's, `.full` the wrapped target
    (monitoring on all rows: elbo_batch(flow, mb.full, xs)).  `resample(stream)` draws the batch of stream index `stream` under `seed`;
    the object is constructed resampled at stream 0.  train_flow resamples before each step with the stream index of that step's
    draws; elbo_batch and value_and_gradient called directly use the current batch.  Under a communicator every rank passes the same
    seed, so that all ranks see the same rows.  unpack, predict, coefficients, scales, dispersion and weights are the full target's."""

    _DELEGATED = ("unpack", "predict", "coefficients", "scales", "dispersion", "weights")

    def __init__(self, target, batch_rows, seed=0):
        segs, wseg, w = minibatch_segments(target)
        if isinstance(batch_rows, bool) or not hasattr(batch_rows, "__index__") or not 1 <= int(batch_rows) <= target.rows:
            raise NFHipError(f"MinibatchTarget: batch_rows must be an integer in 1..{target.rows}")
        if isinstance(seed, bool) or not hasattr(seed, "__index__") or not 0 <= int(seed) < 2**64:
            raise NFHipError("MinibatchTarget: seed must be an integer in 0..2^64-1")
        if target.A.device.type != "cuda":
            raise NFHipError("MinibatchTarget: the batch is gathered on the device: build the target from device tensors")
        m = int(batch_rows)
        self.full, self.d, self.rows, self.seed = target, target.d, m, int(seed)
        self.A = torch.empty((m, w), dtype=target.A.dtype, device=target.A.device)
        self.p0 = torch.empty(sum(m if per_row else n for per_row, n in segs), dtype=target.p0.dtype, device=target.p0.device)
        self.idx = torch.empty(m, dtype=torch.int32, device=target.A.device)
        self.c = Target()
        self.resample(0)

    def __getattr__(self, name):  # (only reached for names the object does not have)
        if name in MinibatchTarget._DELEGATED and "full" in self.__dict__:
            return getattr(self.full, name)
        raise AttributeError(f"{type(self).__name__!r} object has no attribute {name!r}")

    def resample(self, stream, indices=None):
        """Draw the batch of stream index `stream` (asynchronous, ordered before any later library call on the device's context) and
        return self.  `indices` (batch_rows integers) replaces the random draw only: position j still carries the scale n_j of
        stratum j, values outside 0..rows-1 are clamped on the device, and unbiasedness is then the caller's business."""
        full, dev = self.full, self.A.device
        idx_in = None
        if indices is not None:
            idx_in = torch.as_tensor(indices).to(device=dev, dtype=torch.int32).contiguous()
            if idx_in.dim() != 1 or idx_in.numel() != self.rows:
                raise NFHipError(f"MinibatchTarget.resample: indices must hold {self.rows} integers")
        ctx = context_for(dev)
        check(ctx.lib.nf_target_minibatch(ctx.ptr, _dtype_code(self.A.dtype), C.byref(full.c), self.d, full.p0.numel(), self.rows, self.seed,
                                          int(stream) & 0xFFFFFFFF, _ptr(idx_in), _ptr(self.idx), _ptr(self.p0), _ptr(self.A), C.byref(self.c)))
        return self

    @property
    def indices(self):
        """the row of the full target behind every row of the current batch (int32, on the device)"""
        return self.idx


def check_target(target, dtype, device=None, d=None):
    """Element-type / device / dimension agreement between a built-in target and the flow that will read it."""
    if isinstance(target, DiagGaussTarget):
        target.check_compatible(dtype, device if device is not None else target.mu.device, d)
    elif isinstance(target, _LinpredTarget):
        target.check_compatible(dtype, device if device is not None else target.A.device, d)


def target_logp(target, ys: torch.Tensor, with_grad: bool = False):
    ym, vec = as_batch(ys)
    d, n = ym.shape
    check_target(target, ym.dtype, ym.device, d)
    out = torch.empty(n, dtype=ym.dtype, device=ym.device)
    grad = new_batch(d, n, ym.dtype, ym.device) if with_grad else None
    ctx = context_for(ym.device)
    check(ctx.lib.nf_target_logp(ctx.ptr, _dtype_code(ym.dtype), C.byref(target.c), d, n, _ptr(ym), _ptr(out), _ptr(grad)))
    res = out[0] if vec else out
    return (res, grad) if with_grad else res
