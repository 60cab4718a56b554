# RobustGRAPEMI355X.jl -- ccall shim that routes RobustGRAPE.jl's hot path to libgrape.so.
#
# The shim EXTENDS the reference's generic functions (src/RobustGRAPE.jl:9-10) with methods for
# `x::Vector{Float64}` -- more specific than the reference's `x::Vector{<:Real}`
# (UnitaryCalculations.jl:20,180, FidelityCalculations.jl:19,368), so dispatch picks them for every
# Float64 control vector, including the calls the reference makes itself:
#   optimize_fidelity_and_error_sources -> calculate_common! -> calculate_fidelity_and_derivatives
#                                                             (FidelityCalculations.jl:174-216, :177)
#   calculate_fidelity_response(_fft) -> calculate_interaction_error_operators (:246-343)
# so `using RobustGRAPE, RobustGRAPEMI355X` is all a user adds (INTEGRATION.md section 2).  Other
# element types (e.g. Vector{Int}) keep the reference's CPU methods; convert with Float64.(x).
# This is deliberate type piracy on RobustGRAPE's own generics: the shim's purpose is to replace
# their implementation.  The entry points take the reference's own problem structs
# (src/Types.jl:12-56), and an `OperatorBasis` is a `Function`, so it can be stored in their
# `H0::Function`, `Herror::Function` and `target_unitary::Function` fields (Types.jl:13,35,55).
# A FidelityRobustGRAPEProblem whose H0, error sources and target are OperatorBasis objects
# evaluates on the MI355X through include/grape.h; plain closures take the host-table fallback
# (the closures run on the host, the exponentials and traces on the device).  Julia is not
# installed in the build image, so this file is not executed there; the same C entry points are
# exercised from Python by tests/, and tests/test_julia_shim.py checks this file statically.
module RobustGRAPEMI355X

using LinearAlgebra
import RobustGRAPE
using RobustGRAPE: ErrorSource, UnitaryRobustGRAPEProblem, FidelityRobustGRAPEProblem,
                   FidelityRobustGRAPEParameters, optimize_fidelity_and_error_sources
# the reference's generics: methods are ADDED to these (no new functions of the same names)
import RobustGRAPE: calculate_fidelity_and_derivatives, calculate_unitary_and_derivatives,
                    calculate_interaction_error_operators, calculate_expectation_values

# (the re-exported names are RobustGRAPE's own bindings: no clash with `using RobustGRAPE`)
export OperatorTerm, OperatorBasis, grape_expm_batch, plan_sectors, rydberg_full_operator_basis, cz_full_target,
       calculate_fidelity_and_derivatives, calculate_unitary_and_derivatives,
       calculate_interaction_error_operators, calculate_expectation_values,
       optimize_fidelity_and_error_sources

const libgrape = normpath(joinpath(@__DIR__, "..", "robustgrape_amd", "libgrape.so"))
const GRAPE_ABI_VERSION = 12  # include/grape.h

function __init__()
    v = ccall((:grape_abi_version, libgrape), Cint, ())
    v == GRAPE_ABI_VERSION || error("libgrape ABI $v, this shim speaks $GRAPE_ABI_VERSION")
end

# grape_var / grape_func (include/grape.h)
const VAR_ONE, VAR_X, VAR_XADD, VAR_TSTEP = Int32(0), Int32(1), Int32(2), Int32(3)
const FN_ONE, FN_LINEAR, FN_COS, FN_SIN, FN_CIS = Int32(0), Int32(1), Int32(2), Int32(3), Int32(4)

struct GrapeTerm
    op::Int32; var::Int32; index::Int32; func::Int32
    a::Float64; b::Float64; scale_re::Float64; scale_im::Float64
end

struct GrapeDesc
    ndim::Int32; ntimes::Int32; nparam::Int32; nadd::Int32; nerr::Int32; n_ops::Int32
    t0::Float64; eps::Float64; eps2::Float64
    projector_diag::Ptr{Float64}; ops::Ptr{ComplexF64}
    n_h0_terms::Int32; h0_terms::Ptr{GrapeTerm}
    err_term_offsets::Ptr{Int32}; err_terms::Ptr{GrapeTerm}
    n_target_terms::Int32; target_terms::Ptr{GrapeTerm}
    max_batch::Int32; reserved::NTuple{5,Int32}
    projector::Ptr{ComplexF64}   # ABI >= 4: full projector (column-major) or C_NULL (diagonal)
end

# the projector as the descriptor takes it: its diagonal, and the full matrix when P0 is not
# diagonal (FidelityCalculations.jl:47-51 accepts any real matrix)
_pfull(P) = isdiag(P) ? ComplexF64[] : ComplexF64.(P)
_pptr(v) = isempty(v) ? Ptr{ComplexF64}(C_NULL) : pointer(v)

"One coefficient * operator term: scale * f(a*v + b) * op (v = 1, x[index], x_add[index] or nt)."
struct OperatorTerm
    op::Matrix{ComplexF64}
    var::Int32; index::Int32; func::Int32
    a::Float64; b::Float64; scale::ComplexF64
end
OperatorTerm(op; var=VAR_ONE, index=1, func=FN_ONE, a=1.0, b=0.0, scale=1.0) =
    OperatorTerm(ComplexF64.(op), var, Int32(index - 1), func, a, b, ComplexF64(scale))

"""Callable like the reference's closures: H0(nt, x, x_add) / Herror(nt, x, x_add, err) /
target(x_add).  A subtype of `Function`, so it fits the reference's `H0::Function`,
`Herror::Function` and `target_unitary::Function` fields (src/Types.jl:13,35,55)."""
struct OperatorBasis <: Function
    terms::Vector{OperatorTerm}
end
function _coef(t::OperatorTerm, nt, x, x_add)
    v = t.var == VAR_ONE ? 1.0 : t.var == VAR_X ? x[t.index+1] : t.var == VAR_XADD ? x_add[t.index+1] : Float64(nt)
    arg = t.a * v + t.b
    f = t.func == FN_ONE ? 1.0 : t.func == FN_LINEAR ? arg : t.func == FN_COS ? cos(arg) :
        t.func == FN_SIN ? sin(arg) : cis(arg)
    return t.scale * f
end
(B::OperatorBasis)(nt, x, x_add) = sum(_coef(t, nt, x, x_add) * t.op for t in B.terms)
(B::OperatorBasis)(nt, x, x_add, err) = err * sum(_coef(t, nt, x, x_add) * t.op for t in B.terms)
(B::OperatorBasis)(x_add) = sum(_coef(t, 1, Float64[], x_add) * t.op for t in B.terms)

# Operator-basis forms of the reference's d = 9 Rydberg model and CZ target
# (src/RydbergTools.jl:118-130, 197-203), as robustgrape_amd/rydberg.py builds them:
# H(ϕ) = cos ϕ Hc + sin ϕ Hs + Hd, the e^{-iϕ} couplings above the diagonal.
const _FULL_COUPLINGS = ((2, 5, 1), (3, 6, 2), (4, 7, 1), (4, 8, 2), (7, 9, 2), (8, 9, 1))  # (row, col, which Ω)
"rydberg_hamiltonian_full(x[param], Ω1, Ω2, δ1, δ2, B) as an OperatorBasis (RydbergTools.jl:118)."
function rydberg_full_operator_basis(; Ω1::Real=1.0, Ω2::Real=1.0, δ1::Real=0.0, δ2::Real=0.0, B::Real=10.0,
                                     param::Integer=1)
    Hc = zeros(ComplexF64, 9, 9); Hs = zeros(ComplexF64, 9, 9)
    for (r, c, w) in _FULL_COUPLINGS
        s = (w == 1 ? Ω1 : Ω2) / 2
        Hc[r, c] += s; Hc[c, r] += s
        Hs[r, c] += -im * s; Hs[c, r] += im * s
    end
    terms = [OperatorTerm(Hc; var=VAR_X, index=param, func=FN_COS), OperatorTerm(Hs; var=VAR_X, index=param, func=FN_SIN)]
    hd = ComplexF64[0, 0, 0, 0, δ1, δ2, δ1, δ2, δ1 + δ2 + B]
    any(!iszero, hd) && push!(terms, OperatorTerm(Matrix(Diagonal(hd))))
    return OperatorBasis(terms)
end
"cz_with_1q_phase_full(x_add[index]) as an OperatorBasis (RydbergTools.jl:197-203)."
function cz_full_target(; index::Integer=1, rydberg_dimension::Integer=5)
    n = 4 + rydberg_dimension
    e(ks) = Matrix{ComplexF64}(Diagonal([i in ks ? 1.0 : 0.0 for i in 1:n]))
    return OperatorBasis([OperatorTerm(e((1,))),
                          OperatorTerm(e((2, 3)); var=VAR_XADD, index=index, func=FN_CIS),
                          OperatorTerm(e((4,)); var=VAR_XADD, index=index, func=FN_CIS, a=2.0, b=Float64(π))])
end

const GRAPE_ERR_UNSUPPORTED = Cint(-2)  # include/grape.h

"A problem libgrape does not serve (GRAPE_ERR_UNSUPPORTED): the caller takes the reference's CPU method."
struct GrapeUnsupported <: Exception
    msg::String
end

function _check(rc)
    rc == 0 && return nothing
    msg = unsafe_string(ccall((:grape_last_error, libgrape), Cstring, ()))
    rc == GRAPE_ERR_UNSUPPORTED && throw(GrapeUnsupported(msg))
    error("libgrape: " * msg)
end

# The graceful edge of the drop-in: a problem libgrape refuses (d > 64, non-Hermitian closure tables
# above 12 levels, the dense engine's limits -- INTEGRATION.md section 5) is evaluated by the
# reference's own method, reached with `invoke` past this shim's more specific Vector{Float64}
# method (RobustGRAPE's signatures: FidelityCalculations.jl:19,368, UnitaryCalculations.jl:20,180).
# Any other libgrape error still raises.
function _or_reference(device_call, f, sig, args...)
    try
        return device_call()
    catch e
        e isa GrapeUnsupported || rethrow()
        @debug "libgrape does not serve this problem ($(e.msg)); using RobustGRAPE's CPU method"
        return invoke(f, sig, args...)
    end
end

mutable struct DevicePlan
    handle::Ptr{Cvoid}
    keep::Vector{Any}      # arrays the descriptor points into
    nx::Int; nerr::Int
    problem::Any           # the problem the plan was built for (guards the objectid key)
end

# One plan per (problem, nparam, kind): :device (operator-basis fidelity path, max_batch 256),
# :unitary (operator-basis single-x analysis entries, max_batch 1) and :table (closure fallback).
const _plans = Dict{Tuple{UInt,Int,Symbol},DevicePlan}()

function _cached(make, problem, nparam::Int, kind::Symbol)
    key = (objectid(problem), nparam, kind)
    p = get(_plans, key, nothing)
    if p === nothing || p.problem !== problem
        p = make()
        p.problem = problem
        _plans[key] = p
    end
    return p
end

function device_plan(fp::FidelityRobustGRAPEProblem, nparam::Int; device::Integer=0, max_batch::Integer=256,
                     kind::Symbol=:device)
    _cached(fp, nparam, kind) do
        up = fp.unitary_problem
        ops = Matrix{ComplexF64}[]
        tr(terms) = [GrapeTerm((push!(ops, t.op); Int32(length(ops) - 1)), t.var, t.index, t.func,
                               t.a, t.b, real(t.scale), imag(t.scale)) for t in terms]
        h0 = tr(up.H0.terms)
        errs = GrapeTerm[]; offs = Int32[0]
        for es in up.error_sources
            append!(errs, tr(es.Herror.terms)); push!(offs, length(errs))
        end
        tgt = tr(fp.target_unitary.terms)
        opsflat = reduce(vcat, [vec(o) for o in ops])            # column-major, like the C side
        pdiag = Float64.(diag(fp.projector))
        pfull = _pfull(fp.projector)
        keep = Any[opsflat, h0, errs, offs, tgt, pdiag, pfull]
        desc = Ref(GrapeDesc(up.ndim, up.ntimes, nparam, up.nb_additional_param, length(up.error_sources),
                             length(ops), up.t0, up.ϵ, up.ϵ2, pointer(pdiag), pointer(opsflat),
                             length(h0), pointer(h0), pointer(offs), isempty(errs) ? C_NULL : pointer(errs),
                             length(tgt), pointer(tgt), max_batch, ntuple(_ -> Int32(0), 5), _pptr(pfull)))
        out = Ref{Ptr{Cvoid}}(C_NULL)
        GC.@preserve keep begin
            _check(ccall((:grape_plan_create, libgrape), Cint, (Ref{GrapeDesc}, Cint, Ref{Ptr{Cvoid}}),
                         desc, device, out))
        end
        p = DevicePlan(out[], keep, nparam * up.ntimes + up.nb_additional_param, length(up.error_sources), nothing)
        finalizer(q -> ccall((:grape_plan_destroy, libgrape), Cvoid, (Ptr{Cvoid},), q.handle), p)
        p
    end
end

const GRAPE_DESC_HOST_TABLES = Int32(1)
const GRAPE_OPT_GENERAL_H0 = Int32(64)   # include/grape.h: the LU-inverted chain (UnitaryCalculations.jl:47)
const GRAPE_OPT_NO_RANK1 = Int32(65536)  # include/grape.h: the merged gradient walk keeps its matrix state
const GRAPE_OPT_NO_WIDE = Int32(131072)  # include/grape.h: device-resident calls keep the chunked passes
const GRAPE_OPT_TILED_ERR = Int32(262144)  # include/grape.h: error sources on the tiled engine (65-128 levels)

# Closure fallback (grape.h GRAPE_DESC_HOST_TABLES): no operator basis in the descriptor.  The host
# sees H0 only as tables, so `general` (a non-Hermitian nominal H0, e.g. a -iΓ/2 decay term:
# _closure_options) selects the general-H0 path, as robustgrape_amd/engine.py general_h0_for does.
function table_plan(fp::FidelityRobustGRAPEProblem, nparam::Int; device::Integer=0, general::Bool=false)
    _cached(fp, nparam, general ? :table_general : :table) do
        up = fp.unitary_problem
        ne = length(up.error_sources)
        pdiag = Float64.(diag(fp.projector))
        pfull = _pfull(fp.projector)
        opts = general ? GRAPE_OPT_GENERAL_H0 : Int32(0)
        desc = Ref(GrapeDesc(up.ndim, up.ntimes, nparam, up.nb_additional_param, ne, 0, up.t0, up.ϵ, up.ϵ2,
                             pointer(pdiag), C_NULL, 0, C_NULL, C_NULL, C_NULL, 0, C_NULL, 1,
                             (GRAPE_DESC_HOST_TABLES, opts, Int32(0), Int32(0), Int32(0)), _pptr(pfull)))
        out = Ref{Ptr{Cvoid}}(C_NULL)
        GC.@preserve pdiag pfull begin
            _check(ccall((:grape_plan_create, libgrape), Cint, (Ref{GrapeDesc}, Cint, Ref{Ptr{Cvoid}}),
                         desc, device, out))
        end
        p = DevicePlan(out[], Any[pdiag, pfull], nparam * up.ntimes + up.nb_additional_param, ne, nothing)
        finalizer(q -> ccall((:grape_plan_destroy, libgrape), Cvoid, (Ptr{Cvoid},), q.handle), p)
        p
    end
end

# Hermitian within rtol of the largest entry (robustgrape_amd/tables.py is_hermitian_h0); tables
# of shape (d, d, ...)
function _is_hermitian(H::AbstractArray{<:Complex}; rtol::Float64=1e-12)
    isempty(H) && return true
    d = size(H, 1); Hr = reshape(H, d, d, :)
    dev = maximum(abs.(Hr .- conj.(permutedims(Hr, (2, 1, 3)))))
    return dev <= rtol * max(maximum(abs.(Hr)), 1e-300)
end

# Which table plan a closure problem needs (engine.py general_h0_for): the fused kernels chain
# with C_k^-1 = C_k^dagger, so a non-Hermitian nominal H0 takes the general path (up to 12
# levels); above 12 levels every tabulated generator goes through the dense engine's
# interchange-free solve, which needs them Hermitian, so anything else is refused.
function _closure_general(up, H0s::AbstractArray, Hall::AbstractArray)
    if up.ndim > 12
        _is_hermitian(Hall) || throw(GrapeUnsupported("closure problems above 12 levels need Hermitian H0 / H0 + " *
                                                      "Herror tables (the dense engine's exponential)"))
        return false
    end
    return !_is_hermitian(H0s)
end

# The closure calls of UnitaryCalculations.jl:45-95 and FidelityCalculations.jl:32-38, tabulated
# in grape_fidelity_grad_tables' variant order (include/grape.h): gradient parameters u = controls
# x[:,k] then x_add, each at +ϵ; with error sources also at +ϵ2, then per error the ϵ / ϵ2 error
# variants and the mixed (u + ϵ2, error ϵ2) ones.
function closure_tables(fp, x::Vector{Float64}, np::Int)
    up = fp.unitary_problem; d, nt, na, ϵ, ϵ2 = up.ndim, up.ntimes, up.nb_additional_param, up.ϵ, up.ϵ2
    errs = up.error_sources; ne = length(errs); n = np + na
    x_main = reshape(x[1:end-na], np, nt); x_add = x[end-na+1:end]
    nv = ne == 0 ? 1 + n : 1 + 2n + ne * (2 + n)
    H = zeros(ComplexF64, d, d, nv, nt)
    for k in 1:nt
        xk = x_main[:, k]
        at(u, δ) = u <= np ? (setindex!(copy(xk), xk[u] + δ, u), copy(x_add)) :
                             (copy(xk), setindex!(copy(x_add), x_add[u-np] + δ, u - np))
        H0k = up.H0(k, copy(xk), copy(x_add))
        H[:, :, 1, k] = H0k
        for u in 1:n
            H[:, :, 1+u, k] = up.H0(k, at(u, ϵ)...)
        end
        ne == 0 && continue
        for u in 1:n
            H[:, :, 1+n+u, k] = up.H0(k, at(u, ϵ2)...)
        end
        for (e, es) in enumerate(errs)
            base = 1 + 2n + (e - 1) * (2 + n)
            H[:, :, base+1, k] = es.Herror(k, copy(xk), copy(x_add), ϵ) + H0k
            H[:, :, base+2, k] = es.Herror(k, copy(xk), copy(x_add), ϵ2) + H0k
            for u in 1:n
                H[:, :, base+2+u, k] = es.Herror(k, at(u, ϵ2)..., ϵ2) + H[:, :, 1+n+u, k]
            end
        end
    end
    U0 = zeros(ComplexF64, d, d, 1 + na)
    U0[:, :, 1] = fp.target_unitary(copy(x_add))
    for q in 1:na
        xa = copy(x_add); xa[q] += ϵ; U0[:, :, 1+q] = fp.target_unitary(xa)
    end
    return H, U0
end

# closure calls of calculate_interaction_error_operators (UnitaryCalculations.jl:193-196)
function closure_interaction_tables(up, x::Vector{Float64}, np::Int)
    d, nt, na, ne = up.ndim, up.ntimes, up.nb_additional_param, length(up.error_sources)
    x_main = reshape(x[1:end-na], np, nt); x_add = x[end-na+1:end]
    H0 = zeros(ComplexF64, d, d, nt); Oerr = zeros(ComplexF64, d, d, ne, nt)
    for k in 1:nt
        H0[:, :, k] = up.H0(k, x_main[:, k], copy(x_add))
        for (e, es) in enumerate(up.error_sources)
            Oerr[:, :, e, k] = (1 / up.ϵ) * es.Herror(k, x_main[:, k], copy(x_add), up.ϵ)
        end
    end
    return H0, Oerr
end

is_operator_basis(fp::FidelityRobustGRAPEProblem) =
    fp.unitary_problem.H0 isa OperatorBasis && fp.target_unitary isa OperatorBasis &&
    all(es.Herror isa OperatorBasis for es in fp.unitary_problem.error_sources)

# The unitary-level entry points take a UnitaryRobustGRAPEProblem (UnitaryCalculations.jl:20,180);
# the descriptor needs a projector and a target, neither of which enters their outputs: wrap the
# problem with the identity (an OperatorBasis when H0 is one, so the device path serves it).
const _wrapped = Dict{UInt,Tuple{UnitaryRobustGRAPEProblem,FidelityRobustGRAPEProblem}}()
function fidelity_wrapper(problem::UnitaryRobustGRAPEProblem)
    w = get(_wrapped, objectid(problem), nothing)
    w !== nothing && w[1] === problem && return w[2]
    d = problem.ndim
    eye = Matrix{ComplexF64}(I, d, d)
    ob = problem.H0 isa OperatorBasis && all(es.Herror isa OperatorBasis for es in problem.error_sources)
    target = ob ? OperatorBasis([OperatorTerm(eye)]) : (x_add -> eye)
    fp = FidelityRobustGRAPEProblem(unitary_problem=problem, projector=Matrix{Float64}(I, d, d), target_unitary=target)
    _wrapped[objectid(problem)] = (problem, fp)
    return fp
end

"Drop-in for src/FidelityCalculations.jl:19-119: (F, F_dx_tot, F_d2err, F_d2err_dx_tot)."
calculate_fidelity_and_derivatives(fp::FidelityRobustGRAPEProblem, x::Vector{Float64}) =
    _or_reference(() -> _device_fidelity(fp, x), calculate_fidelity_and_derivatives,
                  Tuple{FidelityRobustGRAPEProblem,Vector{<:Real}}, fp, x)

"Drop-in for src/UnitaryCalculations.jl:20-155: (U, U_dx, U_dx_add, U_derr, U_derr_dx, U_derr_dx_add)."
calculate_unitary_and_derivatives(problem::UnitaryRobustGRAPEProblem, x::Vector{Float64}) =
    _or_reference(() -> _device_unitary(problem, x), calculate_unitary_and_derivatives,
                  Tuple{UnitaryRobustGRAPEProblem,Vector{<:Real}}, problem, x)

"Drop-in for src/UnitaryCalculations.jl:180-204: (ndim, ndim, ntimes, nerr)."
calculate_interaction_error_operators(problem::UnitaryRobustGRAPEProblem, x::Vector{Float64}) =
    _or_reference(() -> _device_interaction(problem, x), calculate_interaction_error_operators,
                  Tuple{UnitaryRobustGRAPEProblem,Vector{<:Real}}, problem, x)

"Drop-in for src/FidelityCalculations.jl:368-390: (ntimes, nerr)."
calculate_expectation_values(fp::FidelityRobustGRAPEProblem, x::Vector{Float64}) =
    _or_reference(() -> _device_expectation(fp, x), calculate_expectation_values,
                  Tuple{FidelityRobustGRAPEProblem,Vector{<:Real}}, fp, x)

# device bodies of the four entry points (GrapeUnsupported escapes to _or_reference)
function _device_fidelity(fp::FidelityRobustGRAPEProblem, x::Vector{Float64})
    up = fp.unitary_problem
    up.ndim > 64 && throw(GrapeUnsupported("ndim > GRAPE_MAX_DENSE_DIM (64)"))
    xm = length(x) - up.nb_additional_param
    @assert mod(xm, up.ntimes) == 0 "Control parameter size must be a multiple of time steps"
    if !is_operator_basis(fp)          # closure fallback
        np = xm ÷ up.ntimes
        xv = Vector{Float64}(x)
        H, U0 = closure_tables(fp, xv, np)
        p = table_plan(fp, np; general=_closure_general(up, H[:, :, 1, :], H))
        F = Ref{Float64}(0.0); F_dx = zeros(p.nx); F_d2err = zeros(p.nerr); F_d2err_dx = zeros(p.nx, p.nerr)
        GC.@preserve xv H U0 F_dx F_d2err F_d2err_dx begin
            _check(ccall((:grape_fidelity_grad_tables, libgrape), Cint,
                         (Ptr{Cvoid}, Cint, Ptr{Float64}, Ptr{ComplexF64}, Ptr{ComplexF64}, Ref{Float64},
                          Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                         p.handle, 1, xv, H, U0, F, F_dx, F_d2err, F_d2err_dx))
        end
        return (F[], F_dx, F_d2err, F_d2err_dx)
    end
    p = device_plan(fp, xm ÷ up.ntimes)
    xv = Vector{Float64}(x)
    F = Ref{Float64}(0.0); F_dx = zeros(p.nx); F_d2err = zeros(p.nerr); F_d2err_dx = zeros(p.nx, p.nerr)
    GC.@preserve xv F_dx F_d2err F_d2err_dx begin
        _check(ccall((:grape_fidelity_grad, libgrape), Cint,
                     (Ptr{Cvoid}, Cint, Ptr{Float64}, Ref{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                     p.handle, 1, xv, F, F_dx, F_d2err, F_d2err_dx))
    end
    return (F[], F_dx, F_d2err, F_d2err_dx)
end

function _device_unitary(problem::UnitaryRobustGRAPEProblem, x::Vector{Float64})
    problem.ndim > 64 && throw(GrapeUnsupported("ndim > GRAPE_MAX_DENSE_DIM (64)"))
    fp = fidelity_wrapper(problem)
    up = problem
    d, nt, na, ne = up.ndim, up.ntimes, up.nb_additional_param, length(up.error_sources)
    xm = length(x) - na
    @assert mod(xm, nt) == 0 "Control parameter size must be a multiple of time steps"
    np = xm ÷ nt
    xv = Vector{Float64}(x)
    outs = (zeros(ComplexF64, d, d), zeros(ComplexF64, d, d, np, nt), zeros(ComplexF64, d, d, na),
            zeros(ComplexF64, d, d, ne), zeros(ComplexF64, d, d, np, nt, ne), zeros(ComplexF64, d, d, na, ne))
    if !is_operator_basis(fp)          # closure fallback
        H, _ = closure_tables(fp, xv, np)
        p = table_plan(fp, np; general=_closure_general(up, H[:, :, 1, :], H))
        GC.@preserve xv H outs begin
            _check(ccall((:grape_unitary_derivs_tables, libgrape), Cint,
                         (Ptr{Cvoid}, Ptr{Float64}, Ptr{ComplexF64}, Ptr{ComplexF64}, Ptr{ComplexF64},
                          Ptr{ComplexF64}, Ptr{ComplexF64}, Ptr{ComplexF64}, Ptr{ComplexF64}),
                         p.handle, xv, H, outs...))
        end
        return outs
    end
    p = device_plan(fp, np; max_batch=1, kind=:unitary)
    GC.@preserve xv outs begin
        _check(ccall((:grape_unitary_derivs, libgrape), Cint,
                     (Ptr{Cvoid}, Ptr{Float64}, Ptr{ComplexF64}, Ptr{ComplexF64}, Ptr{ComplexF64},
                      Ptr{ComplexF64}, Ptr{ComplexF64}, Ptr{ComplexF64}), p.handle, xv, outs...))
    end
    return outs
end

function _device_interaction(problem::UnitaryRobustGRAPEProblem, x::Vector{Float64})
    problem.ndim > 64 && throw(GrapeUnsupported("ndim > GRAPE_MAX_DENSE_DIM (64)"))
    fp = fidelity_wrapper(problem)
    up = problem
    np = (length(x) - up.nb_additional_param) ÷ up.ntimes
    xv = Vector{Float64}(x)
    O = zeros(ComplexF64, up.ndim, up.ndim, up.ntimes, length(up.error_sources))
    if !is_operator_basis(fp)          # closure fallback
        H0, Oerr = closure_interaction_tables(up, xv, np)
        p = table_plan(fp, np; general=_closure_general(up, H0, H0))
        GC.@preserve xv H0 Oerr O begin
            _check(ccall((:grape_interaction_error_operators_tables, libgrape), Cint,
                         (Ptr{Cvoid}, Ptr{Float64}, Ptr{ComplexF64}, Ptr{ComplexF64}, Ptr{ComplexF64}, Cint),
                         p.handle, xv, H0, Oerr, O, 0))
        end
        return O
    end
    p = device_plan(fp, np; max_batch=1, kind=:unitary)
    GC.@preserve xv O begin
        _check(ccall((:grape_interaction_error_operators, libgrape), Cint,
                     (Ptr{Cvoid}, Ptr{Float64}, Ptr{ComplexF64}), p.handle, xv, O))
    end
    return O
end

function _device_expectation(fp::FidelityRobustGRAPEProblem, x::Vector{Float64})
    up = fp.unitary_problem
    up.ndim > 64 && throw(GrapeUnsupported("ndim > GRAPE_MAX_DENSE_DIM (64)"))
    np = (length(x) - up.nb_additional_param) ÷ up.ntimes
    xv = Vector{Float64}(x)
    ev = zeros(Float64, up.ntimes, length(up.error_sources))
    if !is_operator_basis(fp)          # closure fallback
        H0, Oerr = closure_interaction_tables(up, xv, np)
        p = table_plan(fp, np; general=_closure_general(up, H0, H0))
        GC.@preserve xv H0 Oerr ev begin
            _check(ccall((:grape_expectation_values_tables, libgrape), Cint,
                         (Ptr{Cvoid}, Ptr{Float64}, Ptr{ComplexF64}, Ptr{ComplexF64}, Ptr{Float64}),
                         p.handle, xv, H0, Oerr, ev))
        end
        return ev
    end
    p = device_plan(fp, np; max_batch=1, kind=:unitary)
    GC.@preserve xv ev begin
        _check(ccall((:grape_expectation_values, libgrape), Cint,
                     (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), p.handle, xv, ev))
    end
    return ev
end

"Batched exp of n column-major d x d ComplexF64 matrices (LinearAlgebra.exp!'s algorithm)."
function grape_expm_batch(As::Vector{Matrix{ComplexF64}}; device::Integer=0)
    d = size(As[1], 1); n = length(As)
    A = reduce(vcat, vec.(As)); E = similar(A); stats = zeros(Int32, 5)
    GC.@preserve A E stats begin
        _check(ccall((:grape_expm_batch, libgrape), Cint,
                     (Cint, Cint, Cint, Ptr{ComplexF64}, Ptr{ComplexF64}, Ptr{Int32}), device, d, n, A, E, stats))
    end
    return [reshape(E[(k-1)*d*d+1:k*d*d], d, d) for k in 1:n], stats
end

"Sector layout of a plan's fidelity path (ABI 5): [(levels, sectors)] per class; [(ndim, 1)] = whole matrices."
function plan_sectors(plan)
    dims = zeros(Cint, 2); nsec = zeros(Cint, 2)
    n = ccall((:grape_plan_sectors, libgrape), Cint, (Ptr{Cvoid}, Ptr{Cint}, Ptr{Cint}, Cint), plan.handle, dims, nsec, 2)
    n < 0 && _check(n)
    return [(Int(dims[c]), Int(nsec[c])) for c in 1:n]
end

end # module
