# NormalizingFlowsNFHipExt -- package extension binding libnfhip.so (MI355X / gfx950, C ABI of include/nfhip.h)
# into NormalizingFlows.jl.  Modelled on ext/NormalizingFlowsCUDAExt.jl:1-76 of the reference: an extension module
# that adds methods to the generic functions the ELBO / log-likelihood hot path goes through, selected by the device
# RNG type (there: CUDA.RNG; here: NFHipRNG) and by the array type (there: CuArray; here: AMDGPU.ROCArray).
# AMDGPU.jl is used for device memory and the task's HIP stream only -- no CUDA.jl, no compatibility shim.
#
# NOT EXECUTED in the build image (no Julia there).  The same ABI is exercised call for call from Python
# (normalizingflows.jl_amd/, tests/test_gpu_parity.py); every ccall signature below is the ctypes signature in
# normalizingflows.jl_amd/_lib.py:SYMBOLS.
#
# Project.toml stanza: ext/Project.toml.stanza
module NormalizingFlowsNFHipExt

using AMDGPU
using NormalizingFlows
using NormalizingFlows: Bijectors, Distributions, Optimisers, ADTypes, Random, LinearAlgebra
using NormalizingFlows: AffineCoupling, NeuralSplineCoupling
import ChainRulesCore

const libnfhip = get(ENV, "NFHIP_LIB", "libnfhip.so")

# ------------------------------------------------------------------------------------------------------------
# C structs of include/nfhip.h (isbits, same field order and padding: five Int32, NTuple{4,Int32}, Int32, Float32, Ptr)
# ------------------------------------------------------------------------------------------------------------
struct NFDesc
    kind::Int32
    dtype::Int32
    d::Int32
    nlayers::Int32
    n_hidden::Int32
    hdims::NTuple{4,Int32}
    K::Int32
    B::Float32
    score::Ptr{Cvoid}   # NF_KIND_HAMILTONIAN: pointer to the NFTarget behind LeapFrog's score, else C_NULL
    base::Ptr{Cvoid}    # pointer to an NFBase for a general MvNormal(mu, Sigma) q0, C_NULL = MvNormal(zeros, I)
    nsegments::Int32    # NF_KIND_COMPOSITE: mixed bijector families, see segments_of
    segments::Ptr{Cvoid}
end
struct NFBase            # nf_base: kind 1 = Diagonal(sigma^2) (scale = sigma), 2 = dense (scale = L, column-major)
    kind::Int32
    mu::Ptr{Cvoid}
    scale::Ptr{Cvoid}
    logdet::Float64
end
struct NFTarget
    kind::Int32
    p0::Ptr{Cvoid}
    p1::Ptr{Cvoid}
    s0::Float64
    s1::Float64
end

const NF_KIND_PLANAR, NF_KIND_RADIAL, NF_KIND_REALNVP, NF_KIND_NSF, NF_KIND_MEANFIELD = Int32(0), Int32(1), Int32(2), Int32(3), Int32(4)
const NF_TARGET_DIAGGAUSS, NF_TARGET_BANANA, NF_TARGET_FUNNEL, NF_TARGET_WARPED, NF_TARGET_CROSS = Int32(0), Int32(1), Int32(2), Int32(3), Int32(4)
const NF_TARGET_DENSEGAUSS, NF_TARGET_LOGREG = Int32(5), Int32(6)   # linear-predictor targets (nfhip.h)
const NF_TARGET_GAUSSMIX = Int32(8)                                  # Gaussian mixture (nfhip.h; kind 7 is unassigned)
# generalised linear-predictor targets (nfhip.h): row offsets, row weights, a linear term, a family parameter
const NF_TARGET_GLM_LOGIT, NF_TARGET_GLM_PROBIT, NF_TARGET_GLM_POISSON, NF_TARGET_GLM_STUDENT, NF_TARGET_GLM_NORMAL =
    Int32(9), Int32(10), Int32(11), Int32(12), Int32(13)
const NF_TARGET_HGLM_OFFSET = Int32(7)                                # hierarchical GLM kinds 16..20 = the GLM kind + 7 (nfhip.h)
const NF_TARGET_SOFTMAX = Int32(15)                                  # softmax regression (nfhip.h; kind 14 is unassigned)
# one-hidden-layer Bayesian neural-network targets (nfhip.h): the GLM kind + 13; kind 21 is unassigned
const NF_TARGET_BNN_LOGIT, NF_TARGET_BNN_PROBIT, NF_TARGET_BNN_POISSON, NF_TARGET_BNN_STUDENT, NF_TARGET_BNN_NORMAL =
    Int32(22), Int32(23), Int32(24), Int32(25), Int32(26)
# GLM targets with a learned dispersion (nfhip.h): y = [β ; τ ; λ]; kinds 27 and 28 are unassigned
const NF_TARGET_DGLM_NORMAL, NF_TARGET_DGLM_STUDENT, NF_TARGET_DGLM_NEGBIN =
    Int32(29), Int32(30), Int32(31)
const NF_TARGET_ORDINAL_LOGIT = Int32(32)                             # ordinal (cumulative-logit) regression (nfhip.h)
const NF_TARGET_RISKSET = Int32(33)                                   # risk-set regression: Cox, conditional logit (nfhip.h)
const NF_RISKSET_MAXR = 8192
dtype_code(::Type{Float32}) = Int32(0)
dtype_code(::Type{Float64}) = Int32(1)

function check(code::Integer)
    code == 0 && return nothing
    return error(unsafe_string(ccall((:nf_strerror, libnfhip), Cstring, (Cint,), code)))
end

# ------------------------------------------------------------------------------------------------------------
# context: one nf_ctx per device, enqueueing on the current task's HIP stream
# ------------------------------------------------------------------------------------------------------------
const CONTEXTS = Dict{Int,Ptr{Cvoid}}()

function context()
    dev = AMDGPU.device_id(AMDGPU.device()) - 1          # AMDGPU.jl ids are 1-based, HIP ordinals 0-based
    stream = Ptr{Cvoid}(UInt(AMDGPU.stream().stream.handle))
    ctx = get(CONTEXTS, dev, C_NULL)
    if ctx == C_NULL
        ref = Ref{Ptr{Cvoid}}(C_NULL)
        check(ccall((:nf_ctx_create, libnfhip), Cint, (Cint, Ptr{Cvoid}, Ptr{Ptr{Cvoid}}), dev, stream, ref))
        ctx = CONTEXTS[dev] = ref[]
    else
        check(ccall((:nf_ctx_set_stream, libnfhip), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), ctx, stream))
    end
    return ctx
end

"""
    stash_budget!(bytes)

Bound (bytes ≥ 0; 0 = off) or reset (negative) the activation stash of the RealNVP training steps on the current device:
what Zygote's tape is to `src/optimize.jl:12-14`, kept by the forward kernels for the reverse pass.  Larger batches run in
chunks through the buffer; with 0 the reverse pass recomputes (slower, no extra memory).
"""
stash_budget!(bytes::Integer) =
    check(ccall((:nf_ctx_set_stash_budget, libnfhip), Cint, (Ptr{Cvoid}, Int64), context(), Int64(bytes)))

devptr(A::ROCArray) = Ptr{Cvoid}(UInt(pointer(A)))
devptr(::Nothing) = C_NULL

# ------------------------------------------------------------------------------------------------------------
# the device RNG handle: what CUDA.RNG is to the CUDA extension.  Philox4x32-10 keyed by `seed`; every draw call
# consumes one stream id; `offset` places a shard inside a global batch (multi-GPU).
# ------------------------------------------------------------------------------------------------------------
mutable struct NFHipRNG <: Random.AbstractRNG
    seed::UInt64
    stream::UInt32
    offset::UInt64
end
NFHipRNG(seed::Integer=0; offset::Integer=0) = NFHipRNG(UInt64(seed), UInt32(0), UInt64(offset))
next_stream!(rng::NFHipRNG) = (s = rng.stream; rng.stream += UInt32(1); s)

# ------------------------------------------------------------------------------------------------------------
# desc_of(flow): the static description the library needs, read off flow.transform.
# create_flow composes reduce(∘, Ls) (src/flows/utils.jl:23-26): a left-nested ComposedFunction tree whose leaves,
# left to right, are L1 … Ln -- the order Optimisers.destructure walks (outer before inner), which is the order of
# theta the library expects.
# ------------------------------------------------------------------------------------------------------------
leaves(f::ComposedFunction) = (leaves(f.outer)..., leaves(f.inner)...)
leaves(f) = (f,)

hidden_dims(chain) = Int32[size(l.weight, 1) for l in chain.layers[1:(end - 1)]]

function pad4(h::Vector{Int32})
    length(h) <= 4 || error("nfhip: at most 4 hidden layers")
    return ntuple(i -> i <= length(h) ? h[i] : Int32(0), 4)
end

function desc_of(flow::Bijectors.TransformedDistribution)
    T = eltype(flow.dist)
    d = Int32(length(flow.dist))
    Ls = leaves(flow.transform)
    L1 = first(Ls)
    nohid = ntuple(_ -> Int32(0), 4)
    if all(l -> l isa Bijectors.PlanarLayer, Ls)
        return NFDesc(NF_KIND_PLANAR, dtype_code(T), d, Int32(length(Ls)), 0, nohid, 0, 0.0f0, C_NULL, C_NULL, Int32(0), C_NULL)
    elseif all(l -> l isa Bijectors.RadialLayer, Ls)
        return NFDesc(NF_KIND_RADIAL, dtype_code(T), d, Int32(length(Ls)), 0, nohid, 0, 0.0f0, C_NULL, C_NULL, Int32(0), C_NULL)
    elseif length(Ls) == 2 && Ls[1] isa Bijectors.Shift && Ls[2] isa Bijectors.Scale{<:LinearAlgebra.LowerTriangular}
        # full-rank family: theta = [shift ; the LowerTriangular's parent matrix, column-major] (its upper triangle is never read)
        return NFDesc(NF_KIND_FULLRANK, dtype_code(T), d, Int32(1), 0, nohid, 0, 0.0f0, C_NULL, C_NULL, Int32(0), C_NULL)
    elseif length(Ls) == 2 && Ls[1] isa Bijectors.Shift && Ls[2] isa Bijectors.Scale
        return NFDesc(NF_KIND_MEANFIELD, dtype_code(T), d, Int32(1), 0, nohid, 0, 0.0f0, C_NULL, C_NULL, Int32(0), C_NULL)
    elseif all(l -> l isa AffineCoupling, Ls)
        iseven(length(Ls)) || error("nfhip: realnvp flows are built from RealNVP_layer pairs (src/flows/realnvp.jl:132-145)")
        h = hidden_dims(L1.s)
        return NFDesc(NF_KIND_REALNVP, dtype_code(T), d, Int32(length(Ls) ÷ 2), Int32(length(h)), pad4(h), 0, 0.0f0, C_NULL, C_NULL, Int32(0), C_NULL)
    elseif all(l -> l isa NeuralSplineCoupling, Ls)
        iseven(length(Ls)) || error("nfhip: nsf flows are built from NSF_layer pairs (src/flows/neuralspline.jl:169-184)")
        h = hidden_dims(L1.nn)
        return NFDesc(NF_KIND_NSF, dtype_code(T), d, Int32(length(Ls) ÷ 2), Int32(length(h)), pad4(h), Int32(L1.K), Float32(L1.B), C_NULL, C_NULL, Int32(0), C_NULL)
    end
    return composite_desc(Ls, T, d)   # mixed families: create_flow((L1, …, Ln), q0), src/flows/utils.jl:23-26
end

# Mixed bijector families: maximal runs of one family become the segments of an NF_KIND_COMPOSITE descriptor (flat
# order, first = outermost).  The segment array must outlive the descriptor: SEGMENT_ROOTS owns ONE array per distinct
# segment list (keyed by the segments' own bits -- desc_of runs on every rand / nfhip(flow) call, and a push-only list
# would grow without bound in a sampling loop).
const NF_KIND_COMPOSITE = Int32(6)
const NF_KIND_FULLRANK = Int32(7)
# the non-centring layer of the hierarchical targets over a RealNVP / NSF / full-rank flow (include/nfhip.h; kind 9 is
# unassigned).  The reference has no such bijector: desc_of does not produce this kind, a caller builds the descriptor itself.
const NF_KIND_NONCENTRED = Int32(10)
const SEGMENT_ROOTS = Dict{Vector{NFDesc},Vector{NFDesc}}()
family(l) = l isa Bijectors.PlanarLayer ? :planar : l isa Bijectors.RadialLayer ? :radial : l isa AffineCoupling ? :realnvp :
            l isa NeuralSplineCoupling ? :nsf : error("nfhip: no device kernels for a $(typeof(l)) layer")
function composite_desc(Ls, ::Type{T}, d::Int32) where {T}
    segs = NFDesc[]
    i = 1
    while i <= length(Ls)
        j = i
        while j < length(Ls) && family(Ls[j + 1]) == family(Ls[i]); j += 1; end
        run = Ls[i:j]
        fake = Bijectors.transformed(Distributions.MvNormal(zeros(T, d), LinearAlgebra.I), reduce(∘, run))
        push!(segs, desc_of(fake))          # a single-family run: one of the branches above
        i = j + 1
    end
    segs = get!(SEGMENT_ROOTS, segs, segs)   # the array whose pointer goes into the descriptor stays rooted here
    nohid = ntuple(_ -> Int32(0), 4)
    return NFDesc(NF_KIND_COMPOSITE, dtype_code(T), d, Int32(1), 0, nohid, 0, 0.0f0, C_NULL, C_NULL,
                  Int32(length(segs)), Ptr{Cvoid}(pointer(segs)))
end

# theta: Optimisers.destructure(flow) as is, on the device (src/NormalizingFlows.jl:67)
function theta_of(flow)
    θ, re = Optimisers.destructure(flow)
    θd = θ isa ROCArray ? θ : ROCArray(θ)
    desc = desc_of(flow)
    P = ccall((:nf_param_count, libnfhip), Int64, (Ref{NFDesc},), desc)
    P == length(θd) || error("nfhip: flow has $(length(θd)) parameters, descriptor says $P")
    return θd, re, desc
end

# ------------------------------------------------------------------------------------------------------------
# built-in targets: callable like any `logp`, and recognised by the fused ELBO entry points
# ------------------------------------------------------------------------------------------------------------
abstract type NFHipTarget end
struct DiagGaussTarget{V<:ROCVector} <: NFHipTarget   # logpdf(MvNormal(μ, Diagonal(σ²)), z), test/flow.jl:43-46
    μ::V
    σ²::V
end
struct BananaTarget <: NFHipTarget                    # Banana(d, b, var), example/targets/banana.jl:58-83
    d::Int
    b::Float64
    var::Float64
end
struct FunnelTarget <: NFHipTarget                    # Funnel(d, μ, σ), example/targets/neal_funnel.jl:26-44; Funnel(d) = Funnel(d, 0, 9)
    d::Int
    μ::Float64
    σ::Float64
    function FunnelTarget(d::Integer, μ::Real=0.0, σ::Real=9.0)
        d >= 2 || error("dim must be >= 2")   # neal_funnel.jl:32
        σ > 0 || error("σ must be > 0")       # neal_funnel.jl:33
        return new(d, μ, σ)
    end
end
struct WarpedGaussTarget <: NFHipTarget               # WarpedGauss(σ1, σ2), 2-dimensional, example/targets/warped_gaussian.jl:25-37
    σ1::Float64
    σ2::Float64
    function WarpedGaussTarget(σ1::Real=1.0, σ2::Real=0.12)
        (σ1 > 0 && σ2 > 0) || error("σ₁, σ₂ must be > 0")   # warped_gaussian.jl:31-32
        return new(σ1, σ2)
    end
end
struct CrossTarget <: NFHipTarget                     # Cross(μ, σ), 2-dimensional 4-component mixture, example/targets/cross.jl:29-38
    μ::Float64
    σ::Float64
    function CrossTarget(μ::Real=2.0, σ::Real=0.15)
        σ > 0 || error("σ must be > 0")
        return new(μ, σ)
    end
end
# Linear-predictor targets.  The device reads a ROW-major matrix [rows × d]: a Julia (column-major) d × rows array, i.e.
# the transpose, stored as `At`.  Coupling flows only (nf_elbo_* answer NF_ERR_UNSUPPORTED for planar / radial /
# mean-field / Hamiltonian flows with these kinds).
struct DenseGaussTarget{V<:ROCVector,M<:ROCMatrix} <: NFHipTarget   # logpdf(MvNormal(μ, Σ), z), Σ = L L'
    μ::V
    Wt::M            # transpose of W = inv(L): column-major d × d = W row-major
    logdetW::Float64
end
function DenseGaussTarget(μ::ROCVector{T}, Σ::AbstractMatrix) where {T}
    L = LinearAlgebra.cholesky(LinearAlgebra.Symmetric(Matrix{Float64}(Σ))).L   # throws PosDefException when Σ is not SPD
    W = inv(LinearAlgebra.LowerTriangular(Matrix(L)))
    return DenseGaussTarget(μ, ROCArray(Matrix{T}(transpose(W))), -sum(log, LinearAlgebra.diag(L)))
end
struct LogRegTarget{M<:ROCMatrix,S} <: NFHipTarget   # Bayesian logistic regression, prior N(0, σ² I)
    At::M            # d × n, column i = t_i x_i (row-major n × d for the device)
    σ::Float64
    shift::S         # nothing or a ROCVector (d)
end
function LogRegTarget(X::AbstractMatrix{T}, t::AbstractVector, σ::Real=1.0; shift=nothing) where {T}
    σ > 0 || error("nfhip: prior σ must be > 0")
    s = all(in((-1, 1)), t) ? Float64.(t) : all(in((0, 1)), t) ? 2.0 .* t .- 1.0 : error("nfhip: labels must be in {-1, +1} or {0, 1}")
    size(X, 1) == length(s) || error("nfhip: one label per row of X")
    return LogRegTarget(ROCArray(Matrix{T}(transpose(X .* T.(s)))), Float64(σ), shift)
end
# MixtureModel([MvNormal(μ_k, Σ_k)], π): the W_k = inv(L_k) stacked (row-major K d × d for the device = the column-major
# d × K d array `At` whose block k is transpose(W_k)), and one buffer p0 = m̄ | b | c with m̄ = Σ π_k μ_k,
# b_k = W_k (μ_k − m̄), c_k = log π_k + log|det W_k| − d/2 log 2π.  Factored on the host in Float64; zero-weight components
# are dropped.  Same flows as the linear-predictor targets; Float32 coupling flows need d ≤ 64.
struct GaussMixTarget{V<:ROCVector,M<:ROCMatrix} <: NFHipTarget
    At::M            # d × K d
    p0::V            # d + K d + K
    K::Int
end
function GaussMixTarget(::Type{T}, ws::AbstractVector, μs::AbstractVector, Σs::AbstractVector) where {T}
    (length(ws) == length(μs) == length(Σs) && length(ws) >= 1) || error("nfhip: one weight, mean and covariance per component")
    (all(>=(0), ws) && abs(sum(ws) - 1) <= 1e-6) || error("nfhip: weights must be >= 0 and sum to 1")
    w = Float64.(ws) ./ sum(Float64.(ws))
    keep = findall(>(0), w)
    d = length(μs[1])
    all(k -> length(μs[k]) == d && size(Σs[k]) == (d, d), keep) || error("nfhip: every component needs a length-$d mean and a $d × $d covariance")
    m̄ = zeros(Float64, d)
    for k in keep
        m̄ .+= w[k] .* Float64.(μs[k])
    end
    nk = length(keep)
    At = Matrix{Float64}(undef, d, d * nk)
    b = Matrix{Float64}(undef, d, nk)
    c = Vector{Float64}(undef, nk)
    for (i, k) in enumerate(keep)
        L = LinearAlgebra.cholesky(LinearAlgebra.Symmetric(Matrix{Float64}(Σs[k]))).L   # throws PosDefException for component k
        W = Matrix(inv(LinearAlgebra.LowerTriangular(Matrix(L))))
        At[:, ((i - 1) * d + 1):(i * d)] = transpose(W)
        b[:, i] = W * (Float64.(μs[k]) .- m̄)
        c[i] = log(w[k]) - sum(log, LinearAlgebra.diag(L)) - d / 2 * log(2 * Base.pi)
    end
    return GaussMixTarget(ROCArray(Matrix{T}(At)), ROCArray(Vector{T}(vcat(m̄, vec(b), c))), nk)
end
c_target(t::GaussMixTarget) = NFTarget(NF_TARGET_GAUSSMIX, devptr(t.p0), devptr(t.At), Float64(t.K), 0.0)
function check_target(t::GaussMixTarget, ::Type{T}, d) where {T}
    (eltype(t.At) === T && eltype(t.p0) === T && size(t.At) == (d, d * t.K) && length(t.p0) == d + d * t.K + t.K) ||
        error("nfhip: target must be a $d-dimensional Gaussian mixture in $T")
end
# The generalised form  log p(z) = const + Σ_i wt_i φ(u_i; param) + lin·z − |z|²/(2σ²) − d/2 log(2πσ²),  u = A z + off, with
# family ∈ (:logit, :probit, :poisson, :student, :normal).  The device reads A row-major (the column-major d × rows array `At`)
# and ONE buffer p0 = lin[d] | off[rows] | wt[rows] | (param, const).  σ = Inf is the flat prior.  Same flows as the other
# linear-predictor targets.
struct GLMTarget{V<:ROCVector,M<:ROCMatrix} <: NFHipTarget
    kind::Int32
    At::M            # d × rows
    p0::V            # d + 2 rows + 2
    σ::Float64
end
const GLM_KINDS = Dict(:logit => NF_TARGET_GLM_LOGIT, :probit => NF_TARGET_GLM_PROBIT, :poisson => NF_TARGET_GLM_POISSON,
                       :student => NF_TARGET_GLM_STUDENT, :normal => NF_TARGET_GLM_NORMAL)
function GLMTarget(family::Symbol, A::AbstractMatrix{T}; offset=nothing, weights=nothing, lin=nothing, constant::Real=0.0, param::Real=0.0,
                   σ::Real=1.0) where {T}
    haskey(GLM_KINDS, family) || error("nfhip: family must be one of $(sort(collect(keys(GLM_KINDS))))")
    rows, d = size(A)
    (rows >= 1 && d >= 1 && all(isfinite, A)) || error("nfhip: A must be a finite rows × d matrix")
    off = offset === nothing ? zeros(Float64, rows) : Float64.(offset)
    wt = weights === nothing ? ones(Float64, rows) : Float64.(weights)
    ln = lin === nothing ? zeros(Float64, d) : Float64.(lin)
    (length(off) == rows && length(wt) == rows && length(ln) == d) || error("nfhip: offset and weights have one entry per row, lin one per column")
    (all(isfinite, off) && all(isfinite, ln) && all(w -> isfinite(w) && w >= 0, wt)) || error("nfhip: offsets and lin must be finite, weights finite and >= 0")
    (isfinite(constant) && isfinite(param) && (family !== :student || param > 0)) || error("nfhip: constant and param must be finite, ν > 0")
    (σ > 0 && !isnan(σ)) || error("nfhip: prior σ must be > 0 (Inf: flat prior)")
    p0 = vcat(ln, off, wt, Float64[param, constant])
    return GLMTarget(GLM_KINDS[family], ROCArray(Matrix{T}(transpose(A))), ROCArray(Vector{T}(p0)), Float64(σ))
end
c_target(t::GLMTarget) = NFTarget(t.kind, devptr(t.p0), devptr(t.At), Float64(size(t.At, 2)), t.σ)
function check_target(t::GLMTarget, ::Type{T}, d) where {T}
    (eltype(t.At) === T && eltype(t.p0) === T && size(t.At, 1) == d && length(t.p0) == d + 2 * size(t.At, 2) + 2) ||
        error("nfhip: target must hold $d-dimensional data rows in $T")
end
# Softmax (multinomial-logit) regression over z = vec(W), W the p × C weight matrix (column-major: class-major in z, d = C p):
#   log p(z) = const + Σ_i wt_i (x_i·W[:, c_i] − logsumexp_c x_i·W[:, c]) − |z|²/(2σ²) − d/2 log(2πσ²),  labels c_i ∈ 1:C (Julia's
# 1-based classes; the device reads them 0-based).  The device reads X row-major (the column-major p × rows array `Xt`) and ONE
# buffer p0 = lab[rows] | wt[rows] | (1/σ², const − d/2 log(2πσ²)).  σ = Inf is the flat prior.  Same flows as the GLM targets.
# (Written without a Julia at hand: unrun.)
struct SoftmaxTarget{V<:ROCVector,M<:ROCMatrix} <: NFHipTarget
    Xt::M            # p × rows
    p0::V            # 2 rows + 2
    C::Int
end
function SoftmaxTarget(X::AbstractMatrix{T}, labels::AbstractVector{<:Integer}, C::Integer=maximum(labels); weights=nothing,
                       constant::Real=0.0, σ::Real=1.0) where {T}
    rows, p = size(X)
    (rows >= 1 && p >= 1 && all(isfinite, X)) || error("nfhip: X must be a finite rows × p matrix")
    (2 <= C <= 16 && C * p <= 256) || error("nfhip: 2 <= C <= 16 classes and C p <= 256")
    (length(labels) == rows && all(c -> 1 <= c <= C, labels)) || error("nfhip: one label in 1:C per row")
    wt = weights === nothing ? ones(Float64, rows) : Float64.(weights)
    (length(wt) == rows && all(w -> isfinite(w) && w >= 0, wt)) || error("nfhip: weights have one finite entry >= 0 per row")
    (isfinite(constant) && σ > 0 && !isnan(σ)) || error("nfhip: constant must be finite, prior σ > 0 (Inf: flat prior)")
    d = C * p
    prec, c0 = isinf(σ) ? (0.0, 0.0) : (1 / σ^2, -0.5 * d * log(2π * σ^2))
    p0 = vcat(Float64.(labels .- 1), wt, Float64[prec, constant + c0])
    return SoftmaxTarget(ROCArray(Matrix{T}(transpose(X))), ROCArray(Vector{T}(p0)), Int(C))
end
c_target(t::SoftmaxTarget) = NFTarget(NF_TARGET_SOFTMAX, devptr(t.p0), devptr(t.Xt), Float64(size(t.Xt, 2)), Float64(t.C))
function check_target(t::SoftmaxTarget, ::Type{T}, d) where {T}
    (eltype(t.Xt) === T && eltype(t.p0) === T && t.C * size(t.Xt, 1) == d && length(t.p0) == 2 * size(t.Xt, 2) + 2) ||
        error("nfhip: target must hold $(t.C) classes of $(d ÷ t.C)-dimensional data rows in $T")
end
# One-hidden-layer Bayesian neural network over z = [w_1; …; w_H; v; c] (hidden-unit-major: w_k the p input weights of unit k, v the
# H output weights, c the output bias; d = H (p + 1) + 1):
#   a_ik = tanh(x_i·w_k),  f_i = c + Σ_k v_k a_ik,  u_i = scale_i f_i + offset_i,
#   log p(z) = const + Σ_i wt_i φ(u_i; param) + Σ_k log N(w_k; 0, σh² I) + log N([v; c]; 0, σo² I),  φ the GLM families'.
# scale and offset carry the likelihood (labels ±1 in scale for :logit / :probit, 1/σ and −t/σ for Gaussian or Student noise,
# log-exposures in offset for :poisson).  The device reads X row-major (the column-major p × rows array `Xt`) and ONE buffer
# p0 = scl[rows] | off[rows] | wt[rows] | (param, const + both normalisers, 1/σh², 1/σo²).  σ = Inf is the flat prior.  Same flows
# as the softmax target.  (Written without a Julia at hand: unrun.)
struct BNNTarget{V<:ROCVector,M<:ROCMatrix} <: NFHipTarget
    kind::Int32
    Xt::M            # p × rows
    p0::V            # 3 rows + 4
    H::Int
end
const BNN_KINDS = Dict(:logit => NF_TARGET_BNN_LOGIT, :probit => NF_TARGET_BNN_PROBIT, :poisson => NF_TARGET_BNN_POISSON,
                       :student => NF_TARGET_BNN_STUDENT, :normal => NF_TARGET_BNN_NORMAL)
function BNNTarget(family::Symbol, X::AbstractMatrix{T}, H::Integer; scale=nothing, offset=nothing, weights=nothing, constant::Real=0.0,
                   param::Real=0.0, σhidden::Real=1.0, σout::Real=1.0) where {T}
    haskey(GLM_KINDS, family) || error("nfhip: family must be one of $(sort(collect(keys(GLM_KINDS))))")
    rows, p = size(X)
    (rows >= 1 && p >= 1 && all(isfinite, X)) || error("nfhip: X must be a finite rows × p matrix")
    (1 <= H <= 16 && p <= 128 && H * (p + 1) + 1 <= 256) || error("nfhip: 1 <= H <= 16 hidden units, p <= 128 and H (p + 1) + 1 <= 256")
    scl = scale === nothing ? ones(Float64, rows) : Float64.(scale)
    off = offset === nothing ? zeros(Float64, rows) : Float64.(offset)
    wt = weights === nothing ? ones(Float64, rows) : Float64.(weights)
    (length(scl) == rows && length(off) == rows && length(wt) == rows) || error("nfhip: scale, offset and weights have one entry per row")
    (all(isfinite, scl) && all(isfinite, off) && all(w -> isfinite(w) && w >= 0, wt)) || error("nfhip: scales and offsets must be finite, weights finite and >= 0")
    (isfinite(constant) && isfinite(param) && (family !== :student || param > 0)) || error("nfhip: constant and param must be finite, ν > 0")
    (σhidden > 0 && !isnan(σhidden) && σout > 0 && !isnan(σout)) || error("nfhip: prior σ must be > 0 (Inf: flat prior)")
    fold(σ, n) = isinf(σ) ? (0.0, 0.0) : (1 / σ^2, -0.5 * n * log(2π * σ^2))
    (ph, ch), (po, co) = fold(σhidden, H * p), fold(σout, H + 1)
    p0 = vcat(scl, off, wt, Float64[param, constant + ch + co, ph, po])
    return BNNTarget(BNN_KINDS[family], ROCArray(Matrix{T}(transpose(X))), ROCArray(Vector{T}(p0)), Int(H))
end
c_target(t::BNNTarget) = NFTarget(t.kind, devptr(t.p0), devptr(t.Xt), Float64(size(t.Xt, 2)), Float64(t.H))
function check_target(t::BNNTarget, ::Type{T}, d) where {T}
    (eltype(t.Xt) === T && eltype(t.p0) === T && t.H * (size(t.Xt, 1) + 1) + 1 == d && length(t.p0) == 3 * size(t.Xt, 2) + 4) ||
        error("nfhip: target must hold $(t.H) hidden units over $(size(t.Xt, 1))-dimensional data rows in $T")
end
# Ordinal (cumulative-logit) regression over z = [β (p) ; γ (C − 1)], d = p + C − 1: labels k_i ∈ 0:C-1, η_i = x_i·β + offset_i,
#   c_1 = γ_1, c_k = c_{k−1} + exp(γ_k),  P(k_i) = σ(c_{k_i+1} − η_i) − σ(c_{k_i} − η_i),
#   log p(z) = const + Σ_i wt_i log P(k_i) + log N(β; 0, σβ² I) + Σ_k log N(c_k; cutloc, σc²) + Σ_{k≥2} γ_k.
# The rows are sorted by label (stably) and every label is padded to whole 32-row blocks with rows of weight 0; the device reads the
# padded X row-major (the column-major p × R array `Xt`) and ONE buffer
# p0 = off[R] | wt[R] | lab[R/32] | (1/σβ², const + both normalisers, 1/σc², cutloc) | n_k[C].  σ = Inf is the flat prior.  Same flows
# as the BNN targets.  (Written without a Julia at hand: unrun.)
struct OrdinalRegressionTarget{V<:ROCVector,M<:ROCMatrix} <: NFHipTarget
    Xt::M            # p × R
    p0::V            # 2 R + R/32 + 4 + C
    C::Int
    rows::Int        # the caller's row count
end
function OrdinalRegressionTarget(X::AbstractMatrix{T}, labels::AbstractVector{<:Integer}, C::Integer; offset=nothing, weights=nothing,
                                 σβ::Real=1.0, σc::Real=1.0, cutloc::Real=0.0, constant::Real=0.0) where {T}
    rows, p = size(X)
    (rows >= 1 && p >= 1 && all(isfinite, X)) || error("nfhip: X must be a finite rows × p matrix")
    (2 <= C <= 16 && p + C - 1 <= 256) || error("nfhip: 2 <= C <= 16 categories and p + C - 1 <= 256")
    (length(labels) == rows && all(k -> 0 <= k < C, labels)) || error("nfhip: one label in 0:C-1 per row")
    off = offset === nothing ? zeros(Float64, rows) : Float64.(offset)
    wt = weights === nothing ? ones(Float64, rows) : Float64.(weights)
    (length(off) == rows && length(wt) == rows) || error("nfhip: offset and weights have one entry per row")
    (all(isfinite, off) && all(w -> isfinite(w) && w >= 0, wt)) || error("nfhip: offsets must be finite, weights finite and >= 0")
    (isfinite(constant) && isfinite(cutloc) && σβ > 0 && !isnan(σβ) && σc > 0 && !isnan(σc)) || error("nfhip: constant and cutloc finite, prior σ > 0 (Inf: flat prior)")
    fold(σ, n) = isinf(σ) ? (0.0, 0.0) : (1 / σ^2, -0.5 * n * log(2π * σ^2))
    (pb, cb), (pc, cc) = fold(σβ, p), fold(σc, C - 1)
    order = sortperm(labels; alg=MergeSort)
    counts = [count(==(k), labels) for k in 0:C-1]
    nblk = cld.(counts, 32)
    R = 32 * sum(nblk)
    Xt = zeros(Float64, p, R); offp = zeros(Float64, R); wtp = zeros(Float64, R)
    start = 32 .* (cumsum(nblk) .- nblk); seen = zeros(Int, C)
    for i in order
        k = labels[i] + 1
        r = start[k] + (seen[k] += 1)
        Xt[:, r] = X[i, :]; offp[r] = off[i]; wtp[r] = wt[i]
    end
    blab = Float64[k - 1 for k in 1:C for _ in 1:nblk[k]]
    nk = Float64[sum(wt[labels .== k]; init=0.0) for k in 0:C-1]
    p0 = vcat(offp, wtp, blab, Float64[pb, constant + cb + cc, pc, cutloc], nk)
    return OrdinalRegressionTarget(ROCArray(Matrix{T}(Xt)), ROCArray(Vector{T}(p0)), Int(C), rows)
end
c_target(t::OrdinalRegressionTarget) = NFTarget(NF_TARGET_ORDINAL_LOGIT, devptr(t.p0), devptr(t.Xt), Float64(size(t.Xt, 2)), Float64(t.C))
function check_target(t::OrdinalRegressionTarget, ::Type{T}, d) where {T}
    R = size(t.Xt, 2)
    (eltype(t.Xt) === T && eltype(t.p0) === T && size(t.Xt, 1) + t.C - 1 == d && length(t.p0) == 2 * R + R ÷ 32 + 4 + t.C) ||
        error("nfhip: target must hold $(t.C) categories over $(size(t.Xt, 1))-dimensional data rows in $T")
end
# Risk-set regression (Cox partial likelihood, conditional logit, rankings) over z = β ∈ R^p, the rows ALREADY ordered so that every risk
# set is a prefix of its segment:  η_i = x_i·β + offset_i,  c_i = log Σ_{j ∈ seg(i), j ≤ i} w_j exp(η_j),
#   log p(z) = const + lin·β − Σ_i m_i c_i + log N(β; 0, σ² I).
# The tail is padded to a whole 32-row block with rows of weight 0; the device reads the padded X row-major (the column-major p × R array
# `Xt`) and ONE buffer p0 = off[R] | log w[R] | m[R] | segstart[R] | lin[p] | (1/σ², const + normaliser).  σ = Inf is the flat prior.
# Same flows as the ordinal target.  (Written without a Julia at hand: unrun.)
struct RiskSetTarget{V<:ROCVector,M<:ROCMatrix} <: NFHipTarget
    Xt::M            # p × R
    p0::V            # 4 R + p + 2
    σ::Float64
    rows::Int        # the caller's row count
end
function RiskSetTarget(X::AbstractMatrix{T}, segment_start::AbstractVector, event_mass::AbstractVector; risk_weight=nothing, offset=nothing,
                       lin=nothing, constant::Real=0.0, σ::Real=Inf) where {T}
    rows, p = size(X)
    (rows >= 1 && 1 <= p <= 256) || error("nfhip: X must be a rows × p matrix with 1 <= p <= 256")
    R = 32 * cld(rows, 32)
    R <= NF_RISKSET_MAXR || error("nfhip: at most $NF_RISKSET_MAXR rows")
    w = risk_weight === nothing ? ones(Float64, rows) : Float64.(risk_weight)
    m = Float64.(event_mass)
    off = offset === nothing ? zeros(Float64, rows) : Float64.(offset)
    ln = lin === nothing ? zeros(Float64, p) : Float64.(lin)
    (length(segment_start) == rows && length(m) == rows && length(w) == rows && length(off) == rows && length(ln) == p) ||
        error("nfhip: segment_start, event_mass, risk_weight and offset have one entry per row, lin one per feature")
    (all(v -> isfinite(v) && v >= 0, w) && all(v -> isfinite(v) && v >= 0, m)) || throw(ArgumentError("nfhip: masses and weights must be finite and >= 0"))
    live = w .> 0
    (all(isfinite, X[live, :]) && all(isfinite, off[live]) && all(isfinite, ln)) || throw(ArgumentError("nfhip: non-finite input on a live row"))
    (isfinite(constant) && σ > 0 && !isnan(σ)) || error("nfhip: constant finite, prior σ > 0 (Inf: flat prior)")
    seg = Bool.(segment_start .!= 0); seg[1] = true
    open = false
    for i in 1:rows                                                   # an event mass needs a row of positive weight before it in its segment
        seg[i] && (open = false)
        open |= live[i]
        (m[i] > 0 && !open) && throw(ArgumentError("nfhip: an event mass on a row whose risk set is empty"))
    end
    prec, cn = isinf(σ) ? (0.0, 0.0) : (1 / σ^2, -0.5 * p * log(2π * σ^2))
    Xt = zeros(Float64, p, R); offp = zeros(Float64, R); lw = fill(-Inf, R); mp = zeros(Float64, R); sp = zeros(Float64, R)
    for i in 1:rows
        Xt[:, i] = live[i] ? X[i, :] : map(v -> isfinite(v) ? v : 0.0, X[i, :])
        offp[i] = (live[i] || isfinite(off[i])) ? off[i] : 0.0
        lw[i] = log(w[i]); mp[i] = m[i]; sp[i] = seg[i]
    end
    p0 = vcat(offp, lw, mp, sp, ln, Float64[prec, constant + cn])
    return RiskSetTarget(ROCArray(Matrix{T}(Xt)), ROCArray(Vector{T}(p0)), Float64(σ), rows)
end
c_target(t::RiskSetTarget) = NFTarget(NF_TARGET_RISKSET, devptr(t.p0), devptr(t.Xt), Float64(size(t.Xt, 2)), t.σ)
function check_target(t::RiskSetTarget, ::Type{T}, d) where {T}
    R = size(t.Xt, 2)
    (eltype(t.Xt) === T && eltype(t.p0) === T && size(t.Xt, 1) == d && length(t.p0) == 4 * R + d + 2) ||
        error("nfhip: target must hold $(size(t.Xt, 1))-dimensional data rows in $T")
end
# Hierarchical GLM over z = [β (p coefficients) ; τ (G group log-scales)], d = p + G, centred parameterisation:
#   log p(z) = const + Σ_i wt_i φ(u_i; param) + lin·β + Σ_j log N(β_j; 0, σ_j²) + Σ_g log p(τ_g),  u = Aβ + offset,
#   σ_j = fixedσ[j] where groups[j] == 0 (Inf: flat), exp(τ_g) where groups[j] == g ∈ 1:G (Julia's 1-based groups; the device reads
#   −1 and 0-based).  hyper[g] ∈ (:lognormal, :halfnormal, :halfcauchy): τ_g ~ N(loc, scale²), or exp(τ_g) half-normal / half-Cauchy of
#   that scale as a density over τ_g.  Everything linear in z or constant is folded here in Float64, as the Python mirror does.  The
#   device reads A padded with zero τ-columns, row-major (the column-major d × rows array `At`), and ONE buffer
#   p0 = lin[d] | off[rows] | wt[rows] | (param, const) | grp[p] | isd[p] | hm[G] | his[G] | hk[G] | gptr[G+1] | gidx[p].
# Same flows as the GLM targets.  (Written without a Julia at hand: unrun.)
struct HierarchicalGLMTarget{V<:ROCVector,M<:ROCMatrix} <: NFHipTarget
    kind::Int32
    At::M            # d × rows
    p0::V            # 4 d + 2 rows + 3 + G
    G::Int
end
const HYPER_KINDS = Dict(:lognormal => 0.0, :halfnormal => 1.0, :halfcauchy => 2.0)
function HierarchicalGLMTarget(family::Symbol, A::AbstractMatrix{T}, groups::AbstractVector{<:Integer}, G::Integer; offset=nothing,
                               weights=nothing, lin=nothing, constant::Real=0.0, param::Real=0.0, fixedσ=1.0, hyper=:halfcauchy,
                               hyperloc=0.0, hyperscale=1.0) where {T}
    haskey(GLM_KINDS, family) || error("nfhip: family must be one of $(sort(collect(keys(GLM_KINDS))))")
    rows, p = size(A)
    (rows >= 1 && p >= 1 && all(isfinite, A)) || error("nfhip: A must be a finite rows × p matrix")
    (G >= 0 && p + G <= 256) || error("nfhip: G >= 0 and p + G <= 256")
    (length(groups) == p && all(g -> 0 <= g <= G, groups)) || error("nfhip: one group in 0:G per column (0: a fixed prior scale)")
    d = p + G
    off = offset === nothing ? zeros(Float64, rows) : Float64.(offset)
    wt = weights === nothing ? ones(Float64, rows) : Float64.(weights)
    ln = lin === nothing ? zeros(Float64, p) : Float64.(lin)
    (length(off) == rows && length(wt) == rows && length(ln) == p) || error("nfhip: offset and weights have one entry per row, lin one per column")
    (all(isfinite, off) && all(isfinite, ln) && all(w -> isfinite(w) && w >= 0, wt)) || error("nfhip: offsets and lin must be finite, weights finite and >= 0")
    (isfinite(constant) && isfinite(param) && (family !== :student || param > 0)) || error("nfhip: constant and param must be finite, ν > 0")
    per(v, n) = v isa AbstractVector ? Float64.(v) : fill(Float64(v), n)
    σ, loc, scl = per(fixedσ, p), per(hyperloc, G), per(hyperscale, G)
    hyp = hyper isa Symbol ? fill(hyper, G) : collect(hyper)
    (length(σ) == p && all(s -> s > 0 && !isnan(s), σ)) || error("nfhip: fixedσ must be > 0 (Inf: flat), a scalar or one per column")
    (length(hyp) == G && all(h -> haskey(HYPER_KINDS, h), hyp)) || error("nfhip: hyper must be one of $(sort(collect(keys(HYPER_KINDS)))), or one per group")
    (length(loc) == G && length(scl) == G && all(isfinite, loc) && all(s -> isfinite(s) && s > 0, scl)) || error("nfhip: hyperloc finite, hyperscale finite and > 0")
    L2PI = log(2π)
    c = Float64(constant)
    isd = zeros(Float64, p)
    lintau = zeros(Float64, G)
    for j in 1:p
        if groups[j] > 0
            lintau[groups[j]] -= 1.0
            c -= 0.5 * L2PI
        elseif isfinite(σ[j])
            isd[j] = 1 / σ[j]
            c -= log(σ[j]) + 0.5 * L2PI
        end
    end
    hm, his = zeros(Float64, G), zeros(Float64, G)
    for g in 1:G
        if hyp[g] === :lognormal
            hm[g], his[g] = loc[g], 1 / scl[g]
            c += -log(scl[g]) - 0.5 * L2PI
        else
            hm[g] = log(scl[g])
            lintau[g] += 1.0
            c += (hyp[g] === :halfnormal ? 0.5 : 1.0) * log(2 / π) - hm[g]
        end
    end
    members = [findall(==(g), groups) for g in 1:G]                      # increasing column index
    gptr = Float64.(vcat(0, cumsum(length.(members))))
    gidx = zeros(Float64, p)
    flat = reduce(vcat, members; init=Int[])
    gidx[1:length(flat)] .= flat .- 1
    p0 = vcat(ln, lintau, off, wt, Float64[param, c], Float64.(groups .- 1), isd, hm, his, Float64[HYPER_KINDS[h] for h in hyp], gptr, gidx)
    At = vcat(Matrix{T}(transpose(A)), zeros(T, G, rows))
    return HierarchicalGLMTarget(GLM_KINDS[family] + NF_TARGET_HGLM_OFFSET, ROCArray(At), ROCArray(Vector{T}(p0)), Int(G))
end
c_target(t::HierarchicalGLMTarget) = NFTarget(t.kind, devptr(t.p0), devptr(t.At), Float64(size(t.At, 2)), Float64(t.G))
function check_target(t::HierarchicalGLMTarget, ::Type{T}, d) where {T}
    (eltype(t.At) === T && eltype(t.p0) === T && size(t.At, 1) == d && length(t.p0) == 4 * d + 2 * size(t.At, 2) + 3 + t.G) ||
        error("nfhip: target must hold $d-dimensional data rows ($(d - t.G) coefficients and $(t.G) log-scales) in $T")
end
# GLM with a learned dispersion over z = [β (p) ; τ (G) ; λ], d = p + G + 1: HierarchicalGLMTarget's prior on (β, τ), and
#   family :normal / :student  l_i = φ_fam(u_i e^{-λ}) − λ (σ = exp(λ));  :negbin  l_i = log NB(counts_i; mean exp(u_i), size exp(λ)),
#   exp(λ) under disphyper ∈ (:lognormal, :halfnormal, :halfcauchy) with disploc / dispscale.  counts: integers in 0:4097, required for and
#   only for :negbin.  Folded here in Float64 as the Python mirror does (zero-weight rows enter neither the table nor the folded sums):
#   p0 = lin[d] | off[rows] | wt[rows] | (param, const, Mt, 0) | grp[p] | isd[p] | hm[G+1] | his[G+1] | hk[G+1] | gptr[G+1] | gidx[p] |
#        cnt[rows] | ctab[Mt]   (cnt / ctab: :negbin only; ctab[m] = Σ_{i: k_i > m} wt_i, m = 1:Mt, Mt = max k − 1).
# Same flows as the hierarchical targets.  (Written without a Julia at hand: unrun.)
struct DispersionGLMTarget{V<:ROCVector,M<:ROCMatrix} <: NFHipTarget
    kind::Int32
    At::M            # d × rows
    p0::V
    G::Int
end
const DGLM_KINDS = Dict(:normal => NF_TARGET_DGLM_NORMAL, :student => NF_TARGET_DGLM_STUDENT, :negbin => NF_TARGET_DGLM_NEGBIN)
function DispersionGLMTarget(family::Symbol, A::AbstractMatrix{T}; counts=nothing, groups=nothing, G::Integer=0, offset=nothing,
                             weights=nothing, lin=nothing, constant::Real=0.0, param::Real=0.0, fixedσ=1.0, hyper=:halfcauchy,
                             hyperloc=0.0, hyperscale=1.0, disphyper::Symbol=:halfcauchy, disploc::Real=0.0, dispscale::Real=1.0) where {T}
    haskey(DGLM_KINDS, family) || error("nfhip: family must be one of $(sort(collect(keys(DGLM_KINDS))))")
    rows, p = size(A)
    (rows >= 1 && p >= 1 && all(isfinite, A)) || error("nfhip: A must be a finite rows × p matrix")
    (G >= 0 && p + G + 1 <= 256) || error("nfhip: G >= 0 and p + G + 1 <= 256")
    groups = groups === nothing ? zeros(Int, p) : groups
    (length(groups) == p && all(g -> 0 <= g <= G, groups)) || error("nfhip: one group in 0:G per column (0: a fixed prior scale)")
    ((family === :negbin) == (counts !== nothing)) || error("nfhip: counts are required for, and only for, :negbin")
    d = p + G + 1
    off = offset === nothing ? zeros(Float64, rows) : Float64.(offset)
    wt = weights === nothing ? ones(Float64, rows) : Float64.(weights)
    ln = lin === nothing ? zeros(Float64, p) : Float64.(lin)
    (length(off) == rows && length(wt) == rows && length(ln) == p) || error("nfhip: offset and weights have one entry per row, lin one per column")
    (all(isfinite, off) && all(isfinite, ln) && all(w -> isfinite(w) && w >= 0, wt)) || error("nfhip: offsets and lin must be finite, weights finite and >= 0")
    (isfinite(constant) && isfinite(param) && (family !== :student || param > 0)) || error("nfhip: constant and param must be finite, ν > 0")
    per(v, n) = v isa AbstractVector ? Float64.(v) : fill(Float64(v), n)
    σ = per(fixedσ, p)
    loc, scl = vcat(per(hyperloc, G), Float64(disploc)), vcat(per(hyperscale, G), Float64(dispscale))
    hyp = vcat(hyper isa Symbol ? fill(hyper, G) : collect(hyper), disphyper)
    (length(σ) == p && all(s -> s > 0 && !isnan(s), σ)) || error("nfhip: fixedσ must be > 0 (Inf: flat), a scalar or one per column")
    (length(hyp) == G + 1 && all(h -> haskey(HYPER_KINDS, h), hyp)) || error("nfhip: hyper / disphyper must be one of $(sort(collect(keys(HYPER_KINDS))))")
    (length(loc) == G + 1 && all(isfinite, loc) && all(s -> isfinite(s) && s > 0, scl)) || error("nfhip: locations finite, scales finite and > 0")
    L2PI = log(2π)
    c = Float64(constant)
    isd = zeros(Float64, p)
    lintl = zeros(Float64, G + 1)                                        # lin of [τ ; λ]
    for j in 1:p
        if groups[j] > 0
            lintl[groups[j]] -= 1.0
            c -= 0.5 * L2PI
        elseif isfinite(σ[j])
            isd[j] = 1 / σ[j]
            c -= log(σ[j]) + 0.5 * L2PI
        end
    end
    hm, his = zeros(Float64, G + 1), zeros(Float64, G + 1)
    for g in 1:G+1
        if hyp[g] === :lognormal
            hm[g], his[g] = loc[g], 1 / scl[g]
            c += -log(scl[g]) - 0.5 * L2PI
        else
            hm[g] = log(scl[g])
            lintl[g] += 1.0
            c += (hyp[g] === :halfnormal ? 0.5 : 1.0) * log(2 / π) - hm[g]
        end
    end
    live = findall(>(0), wt)
    tail, Mt = Float64[], 0
    if family === :negbin
        k = Float64.(counts)
        (length(k) == rows && all(x -> isinteger(x) && 0 <= x <= 4097, k)) || error("nfhip: counts must be integers in 0:4097, one per row")
        Mt = isempty(live) ? 0 : max(Int(maximum(k[live])) - 1, 0)
        ctab = Float64[sum(wt[i] for i in live if k[i] > m; init=0.0) for m in 1:Mt]
        logfact(x) = sum(log, 1:Int(x); init=0.0)
        ln = ln .+ vec(transpose(wt[live] .* k[live]) * Float64.(A[live, :]))
        c += sum(wt[i] * (k[i] * off[i] - logfact(k[i])) for i in live; init=0.0)
        tail = vcat(k, ctab)
    else
        lintl[G+1] -= sum(wt[live]; init=0.0)
    end
    members = [findall(==(g), groups) for g in 1:G]                      # increasing column index
    gptr = Float64.(vcat(0, cumsum(length.(members))))
    gidx = zeros(Float64, p)
    flat = reduce(vcat, members; init=Int[])
    gidx[1:length(flat)] .= flat .- 1
    p0 = vcat(ln, lintl, off, wt, Float64[param, c, Mt, 0.0], Float64.(groups .- 1), isd, hm, his, Float64[HYPER_KINDS[h] for h in hyp], gptr, gidx, tail)
    At = vcat(Matrix{T}(transpose(A)), zeros(T, G + 1, rows))
    return DispersionGLMTarget(DGLM_KINDS[family], ROCArray(At), ROCArray(Vector{T}(p0)), Int(G))
end
c_target(t::DispersionGLMTarget) = NFTarget(t.kind, devptr(t.p0), devptr(t.At), Float64(size(t.At, 2)), Float64(t.G))
function check_target(t::DispersionGLMTarget, ::Type{T}, d) where {T}
    (eltype(t.At) === T && eltype(t.p0) === T && size(t.At, 1) == d && length(t.p0) >= 4 * d + 2 * size(t.At, 2) + 5 + t.G) ||
        error("nfhip: target must hold $d-dimensional data rows ($(d - t.G - 1) coefficients, $(t.G) log-scales and the log-dispersion) in $T")
end
# Row minibatch of a regression target for stochastic VI over many rows (nf_target_minibatch, include/nfhip.h): m of the full target's
# rows, gathered on the device into buffers of the full target's own kind and layout -- stratified, one row per stratum, without
# replacement, the weight of row idx_j scaled by the size n_j of its stratum, every host-folded full-data term copied.  An unbiased
# estimate of the full log-density; m = rows is the full target bit for bit.  `resample!(mb, stream)` draws the batch of a stream
# index under `seed`; the constructor resamples at stream 0, train_flow_fused before every step with that step's stream index.
# Every rank of a communicator passes the same seed.  Monitoring on all rows: elbo_batch(flow, mb.full, xs).  Served for GLMTarget,
# SoftmaxTarget, HierarchicalGLMTarget, BNNTarget and DispersionGLMTarget.  (Written without a Julia at hand: unrun.)
const MinibatchFull = Union{GLMTarget,SoftmaxTarget,HierarchicalGLMTarget,BNNTarget,DispersionGLMTarget}
mutable struct MinibatchTarget{F<:MinibatchFull,V<:ROCVector,M<:ROCMatrix} <: NFHipTarget
    full::F
    m::Int
    seed::UInt64
    At::M                 # w × m: the gathered rows
    p0::V
    idx::ROCVector{Int32} # the row of the full target behind every row of the batch
    d::Int
end
rows_matrix(t::Union{GLMTarget,HierarchicalGLMTarget,DispersionGLMTarget}) = t.At
rows_matrix(t::Union{SoftmaxTarget,BNNTarget}) = t.Xt
per_row_segments(::GLMTarget) = 2
per_row_segments(::SoftmaxTarget) = 2
per_row_segments(::HierarchicalGLMTarget) = 2
per_row_segments(::BNNTarget) = 3
per_row_segments(t::DispersionGLMTarget) = t.kind == NF_TARGET_DGLM_NEGBIN ? 3 : 2
target_dim(t::Union{GLMTarget,HierarchicalGLMTarget,DispersionGLMTarget}) = size(t.At, 1)
target_dim(t::SoftmaxTarget) = t.C * size(t.Xt, 1)
target_dim(t::BNNTarget) = t.H * (size(t.Xt, 1) + 1) + 1
function MinibatchTarget(full::MinibatchFull, m::Integer; seed::Integer=0)
    X = rows_matrix(full)
    w, R = size(X)
    1 <= m <= R || error("nfhip: batch_rows must be in 1:$R")
    mb = MinibatchTarget(full, Int(m), UInt64(seed), similar(X, w, m), similar(full.p0, length(full.p0) - per_row_segments(full) * (R - m)),
                         ROCVector{Int32}(undef, m), target_dim(full))
    return resample!(mb, 0)
end
function resample!(mb::MinibatchTarget, stream::Integer; indices::Union{Nothing,ROCVector{Int32}}=nothing)
    indices === nothing || length(indices) == mb.m || error("nfhip: indices must hold $(mb.m) entries")
    out = Ref(NFTarget(Int32(0), C_NULL, C_NULL, 0.0, 0.0))
    check(ccall((:nf_target_minibatch, libnfhip), Cint,
                (Ptr{Cvoid}, Int32, Ref{NFTarget}, Int32, Int64, Int64, UInt64, UInt32, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ref{NFTarget}),
                context(), dtype_code(eltype(mb.p0)), c_target(mb.full), mb.d, length(mb.full.p0), mb.m, mb.seed, UInt32(stream), devptr(indices),
                devptr(mb.idx), devptr(mb.p0), devptr(mb.At), out))
    return mb
end
function c_target(mb::MinibatchTarget)
    f = c_target(mb.full)
    return NFTarget(f.kind, devptr(mb.p0), devptr(mb.At), Float64(mb.m), f.s1)
end
check_target(mb::MinibatchTarget, ::Type{T}, d) where {T} = check_target(mb.full, T, d)
c_target(t::DenseGaussTarget) = NFTarget(NF_TARGET_DENSEGAUSS, devptr(t.μ), devptr(t.Wt), t.logdetW, 0.0)
c_target(t::LogRegTarget) = NFTarget(NF_TARGET_LOGREG, t.shift === nothing ? C_NULL : devptr(t.shift), devptr(t.At), Float64(size(t.At, 2)), t.σ)
function check_target(t::DenseGaussTarget, ::Type{T}, d) where {T}
    (eltype(t.μ) === T && eltype(t.Wt) === T && length(t.μ) == d && size(t.Wt) == (d, d)) || error("nfhip: target must be a length-$d MvNormal in $T")
end
function check_target(t::LogRegTarget, ::Type{T}, d) where {T}
    (eltype(t.At) === T && size(t.At, 1) == d && (t.shift === nothing || (eltype(t.shift) === T && length(t.shift) == d))) ||
        error("nfhip: target must hold $d-dimensional data rows in $T")
end
c_target(t::DiagGaussTarget) = NFTarget(NF_TARGET_DIAGGAUSS, devptr(t.μ), devptr(t.σ²), 0.0, 0.0)
c_target(t::BananaTarget) = NFTarget(NF_TARGET_BANANA, C_NULL, C_NULL, t.b, t.var)
c_target(t::FunnelTarget) = NFTarget(NF_TARGET_FUNNEL, C_NULL, C_NULL, t.μ, t.σ)
c_target(t::WarpedGaussTarget) = NFTarget(NF_TARGET_WARPED, C_NULL, C_NULL, t.σ1, t.σ2)
c_target(t::CrossTarget) = NFTarget(NF_TARGET_CROSS, C_NULL, C_NULL, t.μ, t.σ)
function check_target(t::DiagGaussTarget, ::Type{T}, d) where {T}
    (eltype(t.μ) === T && length(t.μ) == d) || error("nfhip: target must be a length-$d ROCVector{$T} pair")
end
check_target(t::BananaTarget, ::Type, d) = t.d == d || error("nfhip: Banana dimension mismatch")
check_target(t::FunnelTarget, ::Type, d) = t.d == d || error("nfhip: Funnel dimension mismatch")
check_target(t::Union{WarpedGaussTarget,CrossTarget}, ::Type, d) = d == 2 || error("nfhip: WarpedGauss and Cross are 2-dimensional targets")

function (t::NFHipTarget)(ys::ROCMatrix{T}) where {T}
    d, N = size(ys)
    check_target(t, T, d)
    out = ROCVector{T}(undef, N)
    check(ccall((:nf_target_logp, libnfhip), Cint,
                (Ptr{Cvoid}, Int32, Ref{NFTarget}, Int32, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                context(), dtype_code(T), c_target(t), d, N, devptr(ys), devptr(out), C_NULL))
    return out
end

# ------------------------------------------------------------------------------------------------------------
# a4 + a5: _device_specific_rand  (src/NormalizingFlows.jl:94-127; CUDA version ext/NormalizingFlowsCUDAExt.jl:7-48)
# ------------------------------------------------------------------------------------------------------------
function is_standard_normal(s::Distributions.MvNormal)
    return all(iszero, s.μ) && s.Σ isa Union{Distributions.PDMats.ScalMat,Distributions.PDMats.PDiagMat} &&
           all(isone, LinearAlgebra.diag(s.Σ))
end

function NormalizingFlows._device_specific_rand(rng::NFHipRNG, s::Distributions.MvNormal, n::Int)
    T = float(eltype(s))
    d = length(s)
    x = ROCMatrix{T}(undef, d, n)
    bptr, keep = base_of(s, T)     # general MvNormal: μ + L ε on the device, as ext/NormalizingFlowsCUDAExt.jl:43-48 does
    GC.@preserve keep check(ccall((:nf_base_rand, libnfhip), Cint,
                (Ptr{Cvoid}, Int32, Ptr{Cvoid}, Int32, Int64, UInt64, UInt64, UInt32, Ptr{Cvoid}, Ptr{Cvoid}),
                context(), dtype_code(T), bptr, d, n, rng.seed, rng.offset, next_stream!(rng), devptr(x), C_NULL))
    return x
end
NormalizingFlows._device_specific_rand(rng::NFHipRNG, s::Distributions.MvNormal) = vec(NormalizingFlows._device_specific_rand(rng, s, 1))

# rand(rng, flow, n): batched and fused (the CUDA extension maps the transform over columns, :61-74)
function NormalizingFlows._device_specific_rand(rng::NFHipRNG, td::Bijectors.TransformedDistribution, n::Int)
    θ, _, desc = theta_of(td)
    T = eltype(θ)
    y = ROCMatrix{T}(undef, Int(desc.d), n)
    check(ccall((:nf_flow_rand, libnfhip), Cint,
                (Ptr{Cvoid}, Ref{NFDesc}, Ptr{Cvoid}, Int64, UInt64, UInt64, UInt32, Ptr{Cvoid}),
                context(), desc, devptr(θ), n, rng.seed, rng.offset, next_stream!(rng), devptr(y)))
    return y
end
NormalizingFlows._device_specific_rand(rng::NFHipRNG, td::Bijectors.TransformedDistribution) = vec(NormalizingFlows._device_specific_rand(rng, td, 1))

# ------------------------------------------------------------------------------------------------------------
# a6 / a7 / a10 / a12 / a13: with_logabsdet_jacobian on device arrays.
# NFHipTransform carries (theta, desc) so the composed transform is ONE library call instead of a recursion over
# ComposedFunction.  `nfhip(flow)` builds the device flow; flow.transform then is an NFHipTransform.
# ------------------------------------------------------------------------------------------------------------
struct NFHipTransform{V<:ROCVector,R} <: Bijectors.Bijector
    θ::V
    desc::NFDesc
    re::R            # Optimisers restructure: re(θ) gives back the reference-side flow
    inverted::Bool
    keep::Any        # roots what desc points into (the NFBase Ref and its device arrays), or nothing
end
Bijectors.inverse(t::NFHipTransform) = NFHipTransform(t.θ, t.desc, t.re, !t.inverted, t.keep)

# a general MvNormal(μ, Σ) q0 as an nf_base: Σ = L L', scale = σ (diagonal) or L (dense, column-major as Julia stores it)
function base_of(q0::Distributions.MvNormal, ::Type{T}) where {T}
    is_standard_normal(q0) && return C_NULL, nothing
    μ = ROCVector{T}(q0.μ)
    if q0.Σ isa Union{Distributions.PDMats.ScalMat,Distributions.PDMats.PDiagMat}
        σ = ROCVector{T}(sqrt.(LinearAlgebra.diag(q0.Σ)))
        ref = Ref(NFBase(Int32(1), devptr(μ), devptr(σ), Float64(sum(log, Array(σ)))))
        return Base.unsafe_convert(Ptr{Cvoid}, ref), (ref, μ, σ)
    end
    Lh = Matrix{T}(LinearAlgebra.cholesky(Matrix(q0.Σ)).L)
    L = ROCMatrix{T}(Lh)
    ref = Ref(NFBase(Int32(2), devptr(μ), devptr(L), Float64(sum(log, LinearAlgebra.diag(Lh)))))
    return Base.unsafe_convert(Ptr{Cvoid}, ref), (ref, μ, L)
end

with_base(d::NFDesc, base::Ptr{Cvoid}) =
    NFDesc(d.kind, d.dtype, d.d, d.nlayers, d.n_hidden, d.hdims, d.K, d.B, d.score, base, d.nsegments, d.segments)

"nfhip(flow): the same flow with parameters on the device and a library-backed transform"
function nfhip(flow::Bijectors.TransformedDistribution)
    θ, re, desc = theta_of(flow)
    bptr, keep = base_of(flow.dist, eltype(θ))
    return Bijectors.transformed(flow.dist, NFHipTransform(θ, with_base(desc, bptr), re, false, keep))
end

function apply(t::NFHipTransform, x::ROCMatrix{T}) where {T}
    d, N = size(x)
    d == t.desc.d || throw(DimensionMismatch("flow has d=$(t.desc.d), input has $d"))
    y = similar(x)
    ladj = ROCVector{T}(undef, N)
    code = t.inverted ?
        ccall((:nf_flow_inv, libnfhip), Cint, (Ptr{Cvoid}, Ref{NFDesc}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Cvoid}),
              context(), t.desc, devptr(t.θ), devptr(x), N, devptr(y), devptr(ladj)) :
        ccall((:nf_flow_fwd, libnfhip), Cint, (Ptr{Cvoid}, Ref{NFDesc}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Cvoid}),
              context(), t.desc, devptr(t.θ), devptr(x), N, devptr(y), devptr(ladj))
    check(code)
    return y, ladj
end

Bijectors.with_logabsdet_jacobian(t::NFHipTransform, x::ROCMatrix) = apply(t, x)
function Bijectors.with_logabsdet_jacobian(t::NFHipTransform, x::ROCVector)      # vector = one column; scalar logdet
    y, l = apply(t, reshape(x, :, 1))                                             # (src/flows/realnvp.jl:69-75)
    return vec(y), AMDGPU.@allowscalar l[1]
end
Bijectors.transform(t::NFHipTransform, x::ROCVecOrMat) = first(Bijectors.with_logabsdet_jacobian(t, x))
(t::NFHipTransform)(x::ROCVecOrMat) = Bijectors.transform(t, x)

# reverse-mode rule: the mechanism MonotonicSplines uses for its kernels (test/ad.jl:126-127), so AutoZygote works
# for an ARBITRARY logp closure: library forward that keeps its tape (nf_flow_fwd_keep), the closure's own pullback,
# library pullback from that tape (nf_flow_bwd_kept).  The tape is a ROCArray owned by the pullback closure -- the
# device form of the Zygote tape the reference differentiates (src/optimize.jl:12-14 on src/objectives/elbo.jl:65-70);
# the pullback leaves it intact, so calling it twice (jacobians) is fine.
function ChainRulesCore.rrule(::typeof(Bijectors.with_logabsdet_jacobian), t::NFHipTransform, x::ROCMatrix{T}) where {T}
    t.inverted && error("nfhip: the pullback of the inverse chain is exposed through loglikelihood training (AutoNFHip)")
    d, N = size(x)
    d == t.desc.d || throw(DimensionMismatch("flow has d=$(t.desc.d), input has $d"))
    nbytes = ccall((:nf_tape_bytes, libnfhip), Int64, (Ptr{Cvoid}, Ref{NFDesc}, Int64), context(), t.desc, N)
    nbytes < 0 && check(Cint(nbytes))
    tape = ROCVector{UInt8}(undef, nbytes)                       # AMDGPU.jl allocations are 256-byte aligned
    y = similar(x)
    ladj = ROCVector{T}(undef, N)
    check(ccall((:nf_flow_fwd_keep, libnfhip), Cint,
                (Ptr{Cvoid}, Ref{NFDesc}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Csize_t),
                context(), t.desc, devptr(t.θ), devptr(x), N, devptr(y), devptr(ladj), devptr(tape), nbytes))
    function pullback(Δ)
        ȳ, l̄ = ChainRulesCore.unthunk(Δ[1]), ChainRulesCore.unthunk(Δ[2])
        ȳ = ȳ isa ChainRulesCore.AbstractZero ? AMDGPU.zeros(T, size(y)) : ROCMatrix{T}(ȳ)
        l̄ = l̄ isa ChainRulesCore.AbstractZero ? AMDGPU.zeros(T, length(ladj)) : ROCVector{T}(l̄)
        x̄ = similar(x)
        ḡ = similar(t.θ)
        check(ccall((:nf_flow_bwd_kept, libnfhip), Cint,
                    (Ptr{Cvoid}, Ref{NFDesc}, Ptr{Cvoid}, Ptr{Cvoid}, Csize_t, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Cvoid}),
                    context(), t.desc, devptr(t.θ), devptr(tape), nbytes, devptr(ȳ), devptr(l̄), N, devptr(x̄), devptr(ḡ)))
        t̄ = ChainRulesCore.Tangent{typeof(t)}(; θ=ḡ)     # tangent_of: the only differentiable field is θ
        return ChainRulesCore.NoTangent(), t̄, x̄
    end
    return (y, ladj), pullback
end

# logpdf(q0, xs) on the device for the standard normal and for a general MvNormal(μ, Σ) (src/objectives/elbo.jl:6,68)
function Distributions.logpdf(s::Distributions.MvNormal, xs::ROCMatrix{T}) where {T}
    out = ROCVector{T}(undef, size(xs, 2))
    bptr, keep = base_of(s, T)
    GC.@preserve keep check(ccall((:nf_base_logpdf_general, libnfhip), Cint,
                (Ptr{Cvoid}, Int32, Ptr{Cvoid}, Int32, Int64, Ptr{Cvoid}, Ptr{Cvoid}),
                context(), dtype_code(T), bptr, size(xs, 1), size(xs, 2), devptr(xs), devptr(out)))
    return out
end

# ------------------------------------------------------------------------------------------------------------
# a1-a3, a16: objectives with a device RNG and a device flow.  Built-in targets take the fused entry points; any
# other `logp` falls through to the reference's own generic code (src/objectives/elbo.jl:65-97), which then runs on
# the methods above.
# ------------------------------------------------------------------------------------------------------------
const DeviceFlow = Bijectors.TransformedDistribution{<:Any,<:NFHipTransform}

function NormalizingFlows.elbo_batch(rng::NFHipRNG, flow::DeviceFlow, logp::NFHipTarget, n::Int)
    t = flow.transform
    check_target(logp, eltype(t.θ), t.desc.d)
    val = Ref{Float64}(0.0)
    check(ccall((:nf_elbo_batch_rng, libnfhip), Cint,
                (Ptr{Cvoid}, Ref{NFDesc}, Ref{NFTarget}, Ptr{Cvoid}, Int64, UInt64, UInt64, UInt32, Ptr{Float64}),
                context(), t.desc, c_target(logp), devptr(t.θ), n, rng.seed, rng.offset, next_stream!(rng), val))
    return eltype(t.θ)(val[])
end
function NormalizingFlows.elbo_batch(flow::DeviceFlow, logp::NFHipTarget, xs::ROCMatrix)
    t = flow.transform
    val = Ref{Float64}(0.0)
    check(ccall((:nf_elbo_batch, libnfhip), Cint,
                (Ptr{Cvoid}, Ref{NFDesc}, Ref{NFTarget}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Float64}),
                context(), t.desc, c_target(logp), devptr(t.θ), devptr(xs), size(xs, 2), C_NULL, val))
    return eltype(t.θ)(val[])
end
NormalizingFlows.elbo(rng::NFHipRNG, flow::DeviceFlow, logp::NFHipTarget, n::Int) = NormalizingFlows.elbo_batch(rng, flow, logp, n)

function NormalizingFlows.loglikelihood(::Random.AbstractRNG, flow::DeviceFlow, xs::ROCMatrix)
    t = flow.transform
    val = Ref{Float64}(0.0)
    check(ccall((:nf_loglikelihood, libnfhip), Cint,
                (Ptr{Cvoid}, Ref{NFDesc}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Float64}),
                context(), t.desc, devptr(t.θ), devptr(xs), size(xs, 2), C_NULL, val))
    return eltype(t.θ)(val[])
end

# ------------------------------------------------------------------------------------------------------------
# a15: the training step.  AutoNFHip is an ADTypes backend whose "differentiation" is the library's hand-derived
# reverse pass; it plugs into the reference's own loop through the two hooks of src/optimize.jl:8-14.
# train_flow dispatches on the device RNG, exactly as the CUDA extension's methods dispatch on CUDA.RNG.
# ------------------------------------------------------------------------------------------------------------
struct AutoNFHip{V,A} <: ADTypes.AbstractADType
    vo::V                   # elbo, elbo_batch or loglikelihood
    desc::NFDesc
    args::A                 # (logp, n) for the ELBO; (xs,) for loglikelihood
    n_global::Int           # samples over all ranks (== the local n on one GPU)
    comm::Bool              # all-reduce [grad ; loss] over the context's RCCL communicator
end

NormalizingFlows._prepare_gradient(loss, ::AutoNFHip, θ, args...) = nothing

function NormalizingFlows._value_and_gradient(loss, prep, ad::AutoNFHip, θ::ROCVector{T}, rng::NFHipRNG, args...) where {T}
    P = length(θ)
    out = ROCVector{T}(undef, P + 1)                         # [grad ; loss] packed: ONE all-reduce when sharded
    ctx = context()
    if ad.vo === NormalizingFlows.loglikelihood
        xs = ad.args[1]::ROCMatrix{T}
        check(ccall((:nf_loglikelihood_value_and_grad, libnfhip), Cint,
                    (Ptr{Cvoid}, Ref{NFDesc}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}),
                    ctx, ad.desc, devptr(θ), devptr(xs), size(xs, 2), ad.n_global, devptr(out)))
    else
        logp, n = ad.args
        logp isa NFHipTarget || return generic_value_and_gradient(loss, θ, rng, args...)
        check(ccall((:nf_elbo_value_and_grad, libnfhip), Cint,
                    (Ptr{Cvoid}, Ref{NFDesc}, Ref{NFTarget}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, UInt64, UInt64, UInt32, Ptr{Cvoid}),
                    ctx, ad.desc, c_target(logp), devptr(θ), C_NULL, n, ad.n_global, rng.seed, rng.offset, next_stream!(rng), devptr(out)))
    end
    if ad.comm                                               # sum over ranks, in place, on the context stream
        check(ccall((:nf_allreduce_grad_loss, libnfhip), Cint, (Ptr{Cvoid}, Int32, Ptr{Cvoid}, Int64), ctx, dtype_code(T), devptr(out), P + 1))
    end
    ls = AMDGPU.@allowscalar out[P + 1]
    return ls, view(out, 1:P)
end

# arbitrary `logp` closure: reverse-mode AD of the reference's own loss through the rrule above
function generic_value_and_gradient(loss, θ, rng, args...)
    Zygote = Base.require(Base.PkgId(Base.UUID("e88e6eb3-aa80-5325-afca-941959d7151f"), "Zygote"))
    ls, back = Zygote.pullback(th -> loss(th, rng, args...), θ)
    return ls, first(back(one(ls)))
end

function NormalizingFlows.train_flow(rng::NFHipRNG, vo, flow::Bijectors.TransformedDistribution, args...;
                                     max_iters::Int=1000, optimiser::Optimisers.AbstractRule=Optimisers.ADAM(),
                                     ADbackend=nothing, n_global::Int=0, allreduce::Bool=false, kwargs...)
    dflow = flow isa DeviceFlow ? flow : nfhip(flow)
    t = dflow.transform
    θ = copy(t.θ)
    re_dev = th -> Bijectors.transformed(dflow.dist, NFHipTransform(th, t.desc, t.re, false, t.keep))   # t.desc is static
    loss(th, rng_, args_...) = -vo(rng_, re_dev(th), args_...)
    nloc = vo === NormalizingFlows.loglikelihood ? size(args[1], 2) : args[2]
    ad = AutoNFHip(vo, t.desc, args, n_global > 0 ? n_global : nloc, allreduce)
    θ_trained, opt_stats, st = NormalizingFlows.optimize(ad, loss, θ, re_dev, rng, args...;
                                                        max_iters=max_iters, optimiser=optimiser, kwargs...)
    return re_dev(θ_trained), opt_stats, st
end

# ------------------------------------------------------------------------------------------------------------
# (e) multi-GPU: sample shards + ONE all-reduce of [grad ; loss] per step (include/nfhip.h, "multi-GPU").
# One Julia process per GPU (as with MPI.jl launchers): rank 0 creates the id, the launcher's own channel ships the
# 128 bytes, every rank joins; then train_flow(NFHipRNG(seed; offset = rank * n), ...; n_global = nranks * n,
# allreduce = true).  Single process, G devices: nf_comm_init_all over the G contexts + nf_allreduce_grad_loss_all.
# ------------------------------------------------------------------------------------------------------------
function comm_unique_id()
    id = zeros(UInt8, 128)
    check(ccall((:nf_comm_get_unique_id, libnfhip), Cint, (Ptr{UInt8},), id))
    return id
end
comm_init_rank(id::Vector{UInt8}, nranks::Integer, rank::Integer) =
    check(ccall((:nf_comm_init_rank, libnfhip), Cint, (Ptr{Cvoid}, Ptr{UInt8}, Int32, Int32), context(), id, nranks, rank))
comm_destroy() = check(ccall((:nf_comm_destroy, libnfhip), Cint, (Ptr{Cvoid},), context()))
# ABI v4: the step's one logical all-reduce may travel in buckets of whole couplings on a second stream (large gradients only,
# 4 MiB by default); bytes < 0 automatic, 0 one message.  comm_bucket_count(flow): messages nf_elbo_step issues per step.
comm_bucket_bytes!(bytes::Integer) =
    check(ccall((:nf_ctx_set_comm_bucket_bytes, libnfhip), Cint, (Ptr{Cvoid}, Int64), context(), bytes))
comm_bucket_count(flow::DeviceFlow) =
    ccall((:nf_comm_bucket_count, libnfhip), Cint, (Ptr{Cvoid}, Ref{NFDesc}), context(), flow.transform.desc)

# ------------------------------------------------------------------------------------------------------------
# ABI v4: the whole iteration of src/optimize.jl:85-99 in ONE call (nf_elbo_step: draws, forward, reverse pass, [all-reduce,]
# Adam, norm(g)) -- what bench.py times and what the Python mirror's train_flow runs for built-in targets.  The loop owns θ
# between iterations, so it may opt in to the library's packed-weight cache (nf_ctx_set_weight_cache) and must opt out when
# it returns; by default every nf_elbo_step packs from θ, so a θ edited or re-allocated behind the library's back is safe.
# ------------------------------------------------------------------------------------------------------------
weight_cache!(on::Bool) = check(ccall((:nf_ctx_set_weight_cache, libnfhip), Cint, (Ptr{Cvoid}, Int32), context(), on ? 1 : 0))
weights_changed!() = check(ccall((:nf_ctx_weights_changed, libnfhip), Cint, (Ptr{Cvoid},), context()))

function elbo_step!(θ::ROCVector{T}, m::ROCVector{T}, v::ROCVector{T}, desc::NFDesc, logp::NFHipTarget, n::Integer, rng::NFHipRNG,
                    step::Integer, rule::Optimisers.Adam) where {T}
    loss, gnorm = Ref{Cdouble}(0), Ref{Cdouble}(0)
    check(ccall((:nf_elbo_step, libnfhip), Cint,
                (Ptr{Cvoid}, Ref{NFDesc}, Ref{NFTarget}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, UInt64, UInt32,
                 Cdouble, Cdouble, Cdouble, Cdouble, Ref{Cdouble}, Ref{Cdouble}),
                context(), desc, c_target(logp), devptr(θ), devptr(m), devptr(v), n, rng.seed, step,
                rule.eta, rule.beta[1], rule.beta[2], rule.epsilon, loss, gnorm))
    return loss[], gnorm[]
end

# train_flow_fused(rng, flow, logp, n; max_iters, optimiser::Adam, state): the fused loop for a built-in target (same numbers as
# train_flow over AutoNFHip; tests/test_gpu_tape.py checks that equality through the Python mirror of this function,
# objectives._optimize_fused / _fused_steps_apply).
# nf_elbo_step uses ONE index for the Philox stream of the draws and for Adam's step count t - 1, and draws from sample offset
# 0 of a single-rank context.  So the fused loop applies only when the two are in step -- a fresh rng (stream 0) with a fresh
# state, or an rng and a `state` continued together (rng.stream == state.t) -- with rng.offset == 0 and no communicator on the
# context; anything else is refused here and belongs to train_flow over AutoNFHip (ADVICE r4: an rng that had already drawn
# started Adam at t = stream + 1 with m = v = 0, and the offset was dropped).  A non-finite loss is recorded, not thrown, as
# the reference's loop would record it (src/optimize.jl:85-99); the returned state carries the real step count.
const NF_ERR_NONFINITE = Cint(-4)  # include/nfhip.h
comm_size() = ccall((:nf_comm_size, libnfhip), Cint, (Ptr{Cvoid},), context())
function fused_steps_apply(rng::NFHipRNG, state)
    t0 = state === nothing ? 0 : Int(state.t)
    return rng.offset == 0 && Int(rng.stream) == t0 && comm_size() <= 1
end
function train_flow_fused(rng::NFHipRNG, flow::Bijectors.TransformedDistribution, logp::NFHipTarget, n::Integer;
                          max_iters::Int=1000, optimiser::Optimisers.Adam=Optimisers.Adam(), state=nothing)
    fused_steps_apply(rng, state) ||
        error("nfhip: train_flow_fused needs rng.stream == state.t (0 for a fresh run), rng.offset == 0 and a single-rank context; use train_flow(rng, elbo_batch, flow, logp, n; ADbackend = AutoNFHip(...)) otherwise")
    dflow = flow isa DeviceFlow ? flow : nfhip(flow)
    t = dflow.transform
    θ = copy(t.θ)
    m = state === nothing ? zero(θ) : copy(state.m)
    v = state === nothing ? zero(θ) : copy(state.v)
    steps = state === nothing ? 0 : Int(state.t)
    stats = NamedTuple[]
    weight_cache!(true)
    try
        for i in 1:max_iters
            loss, gnorm = Ref{Cdouble}(0), Ref{Cdouble}(0)
            s = next_stream!(rng)
            logp isa MinibatchTarget && resample!(logp, s)   # this step's rows, under the stream index of this step's draws
            code = ccall((:nf_elbo_step, libnfhip), Cint,
                         (Ptr{Cvoid}, Ref{NFDesc}, Ref{NFTarget}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, UInt64, UInt32,
                          Cdouble, Cdouble, Cdouble, Cdouble, Ref{Cdouble}, Ref{Cdouble}),
                         context(), t.desc, c_target(logp), devptr(θ), devptr(m), devptr(v), n, rng.seed, s,
                         optimiser.eta, optimiser.beta[1], optimiser.beta[2], optimiser.epsilon, loss, gnorm)
            code == NF_ERR_NONFINITE || check(code)   # a non-finite loss is recorded
            steps += 1
            push!(stats, (iteration=i, loss=loss[], gradient_norm=gnorm[]))
        end
    finally
        weight_cache!(false)
    end
    return Bijectors.transformed(dflow.dist, NFHipTransform(θ, t.desc, t.re, false, t.keep)), stats, (m=m, v=v, t=steps)
end

# train_flow_fused(flow, loglikelihood, xs; max_iters, optimiser::Adam, state): the forward-KL loop, train_flow(loglikelihood,
# flow, xs) with each iteration ONE nf_loglikelihood_step (value and gradient of -loglikelihood, Adam, norm(g)); same numbers
# as train_flow over AutoNFHip (tests/test_gpu_fkl_step.py checks that through the Python mirror, objectives._optimize_fused_fkl).
# Adam's t - 1 is the step index; there are no draws, so any `state` continues.  Single-rank contexts only: under a
# communicator nf_loglikelihood_step all-reduces inside the library, a data-parallel run of its own.
function train_flow_fused(flow::Bijectors.TransformedDistribution, ::typeof(NormalizingFlows.loglikelihood), xs::ROCMatrix;
                          max_iters::Int=1000, optimiser::Optimisers.Adam=Optimisers.Adam(), state=nothing)
    comm_size() <= 1 || error("nfhip: train_flow_fused needs a single-rank context")
    dflow = flow isa DeviceFlow ? flow : nfhip(flow)
    t = dflow.transform
    θ = copy(t.θ)
    ys = convert(ROCMatrix{eltype(θ)}, xs)
    N = Int64(size(ys, 2))
    m = state === nothing ? zero(θ) : copy(state.m)
    v = state === nothing ? zero(θ) : copy(state.v)
    steps = state === nothing ? 0 : Int(state.t)
    stats = NamedTuple[]
    weight_cache!(true)
    try
        for i in 1:max_iters
            loss, gnorm = Ref{Cdouble}(0), Ref{Cdouble}(0)
            code = ccall((:nf_loglikelihood_step, libnfhip), Cint,
                         (Ptr{Cvoid}, Ref{NFDesc}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, UInt32,
                          Cdouble, Cdouble, Cdouble, Cdouble, Ref{Cdouble}, Ref{Cdouble}),
                         context(), t.desc, devptr(θ), devptr(m), devptr(v), devptr(ys), N, N, UInt32(steps),
                         optimiser.eta, optimiser.beta[1], optimiser.beta[2], optimiser.epsilon, loss, gnorm)
            code == NF_ERR_NONFINITE || check(code)   # a non-finite loss is recorded
            steps += 1
            push!(stats, (iteration=i, loss=loss[], gradient_norm=gnorm[]))
        end
    finally
        weight_cache!(false)
    end
    return Bijectors.transformed(dflow.dist, NFHipTransform(θ, t.desc, t.re, false, t.keep)), stats, (m=m, v=v, t=steps)
end

# The capturable form (hipGraph): Adam's t - 1 lives in `counter` (device UInt32), which the step increments; `out` (2 elements,
# optional) receives [loss ; norm(g)].  NF_ERR_UNSUPPORTED (an error here) for flows without the fused form.
function loglikelihood_step_enqueue!(θ::ROCVector{T}, m::ROCVector{T}, v::ROCVector{T}, desc::NFDesc, ys::ROCMatrix{T},
                                     counter::ROCVector{UInt32}, rule::Optimisers.Adam, out=nothing) where {T}
    N = Int64(size(ys, 2))
    check(ccall((:nf_loglikelihood_step_enqueue, libnfhip), Cint,
                (Ptr{Cvoid}, Ref{NFDesc}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid},
                 Cdouble, Cdouble, Cdouble, Cdouble, Ptr{Cvoid}),
                context(), desc, devptr(θ), devptr(m), devptr(v), devptr(ys), N, N, devptr(counter),
                rule.eta, rule.beta[1], rule.beta[2], rule.epsilon, devptr(out)))
    return nothing
end

end # module
