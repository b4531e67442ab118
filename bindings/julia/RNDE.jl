# RNDE.jl -- Julia binding of librnde.so (include/rnde.h) for RegNeuralDE.jl on MI355X.
#
# SOURCE ONLY: no Julia toolchain exists in the build image, so this file has never been executed (INTEGRATION.md says what
# was checked instead: every prototype below is the one regneuralde.jl_amd/_lib.py binds with ctypes and the GPU tests call;
# tests/test_abi.py parses the two config structs below and compares field order, widths and offsets with a C program compiled
# against include/rnde.h, tests/abi_c/abi_check.c, and with the ctypes mirrors).
# It shows exactly what a maintainer adds to the reference: the body of the TrackedNeuralODE call methods between ODEProblem
# construction and result unpacking (reference src/models/neural_ode.jl:126-142) becomes one `ccall`, the same for
# TrackedNeuralDSDE (src/models/neural_sde.jl:98-113), and the reverse sweeps are registered with `Tracker.@grad` so that
# `Tracker.gradient(...)` (reference experiments/mnist_node.jl:229-232) keeps working unchanged.
#
# Device arrays are AMDGPU.jl `ROCArray`s (the reference's `|> gpu` becomes `|> roc`).  A device pointer crosses the ABI as a
# plain `Ptr{Cvoid}`: `devptr(a)` below reinterprets AMDGPU's typed device pointer, nothing else about the array is touched.
module RNDE

import AMDGPU                                   # (binds the module name too: AMDGPU.stream(), AMDGPU.synchronize() below)
import Flux                                     # (NNlib's activations as Flux re-exports them: act_code below)
using AMDGPU: ROCArray, ROCVector, ROCMatrix
using Tracker
using Tracker: TrackedArray, data, track, @grad

const LIB = joinpath(@__DIR__, "..", "..", "regneuralde.jl_amd", "lib", "librnde.so")
const MAX_LAYERS = 8

devptr(a::ROCArray) = reinterpret(Ptr{Cvoid}, pointer(a))

# mirrors rnde_node_config (include/rnde.h); field order and widths must match
struct NodeConfig
    n_layers::Int32
    dims::NTuple{9,Int32}
    act::NTuple{8,Int32}
    time_dep::Int32
    pre_act::Int32
    max_batch::Int32
    solver::Int32
    reltol::Float32
    abstol::Float32
    regularize::Int32
    cb_save_start::Int32
    track_ctrl::Int32
    track_initdt::Int32
    max_attempts::Int32
    device::Int32
    col_tile::Int32
    persist::Int32
    wgrad_side_pct::Int32
    stage_generic::Int32
end

# ---- stream ordering contract ---------------------------------------------------------------------------
# Every entry point below that enqueues work takes the HIP stream of the CURRENT Julia task (AMDGPU.jl arrays live on task-local
# streams): the library's kernels are then ordered against the caller's own array operations on that task, and results read back
# from Julia after the call (or after AMDGPU.synchronize() for the asynchronous ones: backward_async!, classifier_grad!,
# momentum_step!, adam_step!, allreduce_sum!) are complete.  The NULL stream would only be ordered against task streams that
# were created blocking, which AMDGPU.jl does not promise.
function _stream()
    try
        return Base.unsafe_convert(Ptr{Cvoid}, AMDGPU.stream().stream)
    catch
        AMDGPU.synchronize()          # (an AMDGPU.jl without that accessor: fall back to the NULL stream behind a full synchronisation)
        return C_NULL
    end
end

mutable struct Handle
    ptr::Ptr{Cvoid}
    cfg::NodeConfig
    last_nfe::Int
    # tiled = true: rnde_node_create_tiled (include/rnde.h) -- Dense chains wider than 64 whose padded weights fit LDS (tiled_lds_bytes(cfg) <=
    # 160 KB).  By default its reverse pass treats step sizes and times as constants: the config must carry track_ctrl = track_initdt = 0
    # (config_for(...; track = false)), the library refuses anything else by name; set_tracking(h, true, true) then asks for the tracked sweep.
    function Handle(cfg::NodeConfig; tiled::Bool = false)
        out = Ref{Ptr{Cvoid}}(C_NULL)
        st = tiled ? ccall((:rnde_node_create_tiled, LIB), Cint, (Ref{NodeConfig}, Ref{Ptr{Cvoid}}), cfg, out) :
                     ccall((:rnde_node_create, LIB), Cint, (Ref{NodeConfig}, Ref{Ptr{Cvoid}}), cfg, out)
        st == 0 || error(tiled ? "rnde_node_create_tiled: " : "rnde_node_create: ", unsafe_string(ccall((:rnde_last_error, LIB), Cstring, (Ptr{Cvoid},), C_NULL)))
        h = new(out[], cfg, 0)
        finalizer(h -> ccall((:rnde_node_destroy, LIB), Cvoid, (Ptr{Cvoid},), h.ptr), h)
        return h
    end
end

# Which reverse sweep the taped forwards of a TILED handle get (include/rnde.h: rnde_node_set_tracking): (false, false) the default, step sizes
# and times constants; (true, false) the step-size controller differentiated; (true, true) the initial step as well -- the reference's gradient.
# Set after creation (the create config keeps track_ctrl = track_initdt = 0) and while the handle holds no tape.
function set_tracking(h::Handle, track_ctrl::Bool, track_initdt::Bool = false)
    st = ccall((:rnde_node_set_tracking, LIB), Cint, (Ptr{Cvoid}, Int32, Int32), h.ptr, Int32(track_ctrl), Int32(track_initdt))
    st == 0 || error("rnde_node_set_tracking status $st: ", unsafe_string(ccall((:rnde_last_error, LIB), Cstring, (Ptr{Cvoid},), h.ptr)))
    return h
end
function tracking(h::Handle)
    c = Ref{Int32}(0); i = Ref{Int32}(0)
    st = ccall((:rnde_node_tracking, LIB), Cint, (Ptr{Cvoid}, Ref{Int32}, Ref{Int32}), h.ptr, c, i)
    st == 0 || error("rnde_node_tracking status $st")
    return c[] != 0, i[] != 0
end
# Saved points on a TILED handle (include/rnde.h: rnde_node_tiled_reserve_saveat): room for up to max_saveat save times per call switches
# rnde_node_forward_saveat / _everystep on; 0 releases, and the handle refuses them again.  While the handle holds no tape.
function reserve_saveat(h::Handle, max_saveat::Integer)
    st = ccall((:rnde_node_tiled_reserve_saveat, LIB), Cint, (Ptr{Cvoid}, Int32), h.ptr, Int32(max_saveat))
    st == 0 || error("rnde_node_tiled_reserve_saveat status $st: ", unsafe_string(ccall((:rnde_last_error, LIB), Cstring, (Ptr{Cvoid},), h.ptr)))
    return h
end
# 0: a tiled handle without a capacity; -1: a handle of rnde_node_create
saveat_capacity(h::Handle) = Int(ccall((:rnde_node_tiled_saveat_capacity, LIB), Int32, (Ptr{Cvoid},), h.ptr))
# the next forward_saveat on this handle runs along `steps` (2 x n: proposed size, accepted != 0): rnde_debug_arm_replay, a parity instrument
function arm_replay(h::Handle, steps::Matrix{Float32})
    st = ccall((:rnde_debug_arm_replay, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}, Int32), h.ptr, steps, Int32(size(steps, 2)))
    st == 0 || error("rnde_debug_arm_replay status $st")
    return h
end
# (t, dt, dtp_in, EEst, accepted, q) of every attempt of the last solve, 6 x n (rnde_node_attempts_ext)
function attempts_ext(h::Handle)
    n = Ref{Int32}(0)
    out = Matrix{Float32}(undef, 6, h.cfg.max_attempts)
    st = ccall((:rnde_node_attempts_ext, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}, Int32, Ref{Int32}), h.ptr, out, Int32(h.cfg.max_attempts), n)
    st == 0 || error("rnde_node_attempts_ext status $st: ", unsafe_string(ccall((:rnde_last_error, LIB), Cstring, (Ptr{Cvoid},), h.ptr)))
    return out[:, 1:n[]]
end

# LDS bytes of a tile of the tiled engine for this config (no device needed; -1: a malformed shape); the limit is 160 * 1024
tiled_lds_bytes(cfg::NodeConfig) = ccall((:rnde_node_tiled_lds_bytes, LIB), Int64, (Ref{NodeConfig},), cfg)

check(h::Handle, st) = st == 0 ||
    error("rnde status $st: ", unsafe_string(ccall((:rnde_last_error, LIB), Cstring, (Ptr{Cvoid},), h.ptr)))

# ---- which of the library's callbacks a caller's `func` is ------------------------------------------------
# The reference hands the layer a closure, `model(x, p1, p2, p3; func = save_func, ...)` (experiments/mnist_node.jl:134, mnist_nsde.jl), and the
# SavingCallback calls it on the integrator after every accepted step (src/models/neural_ode.jl:126-127).  The library computes the value inside
# its kernels instead, so the closure has to be RECOGNISED, not called per step: it is evaluated on two mock integrators and the two values are
# matched against the reference's own callbacks (mnist_node.jl:67 EEst*dt; :74-79 |eigen_est|/stability_size; :88-97 their blend with 0.1;
# neural_ode.jl:54 the constant 0).  Anything else is refused -- a wrong regulariser must not be trained on silently.
struct MockIntegrator
    EEst::Float32
    dt::Float32
    eigen_est::Float32
end
const REG_NONE, REG_ERR, REG_STIFF, REG_ERR_STIFF, REG_STIFF_DT = 0, 1, 2, 3, 4
const _PROBES = (MockIntegrator(2f0, 3f0, 5f0), MockIntegrator(0.5f0, 0.25f0, -7f0))

"""
    reg_code(func, stability_size) -> REG_NONE | REG_ERR | REG_STIFF | REG_ERR_STIFF | REG_STIFF_DT

`stability_size`: `alg_stability_size` of the solver the experiment divides by (Tsit5: 3.5068, SOSRI2: 10.6).
"""
function reg_code(func, stability_size::Real)
    s = Float64(stability_size)
    got = map(m -> Float64(data(func(nothing, 0f0, m))), _PROBES)
    want = Dict(REG_NONE => m -> 0.0,
                REG_ERR => m -> Float64(m.EEst) * m.dt,
                REG_STIFF => m -> abs(Float64(m.eigen_est)) / s,
                REG_ERR_STIFF => m -> Float64(m.EEst) * m.dt + 0.1 * Float64(m.eigen_est) / s,
                REG_STIFF_DT => m -> abs(Float64(m.eigen_est) * m.dt))      # the reference's own test: abs(integrator.eigen_est * integrator.dt), test/test_node.jl:75,:84
    for code in (REG_NONE, REG_ERR, REG_STIFF, REG_ERR_STIFF, REG_STIFF_DT)
        all(isapprox(g, want[code](m); rtol = 1e-4, atol = 1e-7) for (g, m) in zip(got, _PROBES)) && return code
    end
    error("RNDE: `func` is none of the callbacks librnde.so computes (EEst*dt, |eigen_est|/stability_size, EEst*dt + 0.1*eigen_est/stability_size, |eigen_est*dt|, 0): ",
          "on (EEst, dt, eigen_est) = (2, 3, 5) and (0.5, 0.25, -7) it returned ", got)
end

# the solver object the layer was built with (`n.args[1]`): its name, and whether it is the composite whose steps fill `integrator.eigen_est`
# (AutoTsit5(Tsit5()) / AutoSOSRI2(SOSRI2()): experiments/mnist_node.jl:81,:99, mnist_nsde.jl:60).  Plain algorithms leave eigen_est at 0.
function solver_name(args)
    isempty(args) && return :Tsit5, false
    alg = args[1]
    hasproperty(alg, :algs) && return nameof(typeof(alg.algs[1])), true
    return nameof(typeof(alg)), false
end

# the callback code a (func, solver) pair runs with: `integrator.eigen_est` is filled by the composite solvers only; under a plain one it keeps its initial
# value (1 [RECALL], not 0), so the reference would record a constant there -- every callback that reads it is refused, the blend included
function effective_reg(code::Int, composite::Bool)
    composite && return code
    (code == REG_STIFF || code == REG_STIFF_DT || code == REG_ERR_STIFF) && error("RNDE: `func` reads integrator.eigen_est, which only the composite solvers (AutoTsit5 / AutoSOSRI2) fill; ",
                               "with a plain solver the reference records its initial value, a constant -- build the layer with the composite solver")
    return code
end

# Flux.Dense chain (MLPDynamics / TDChain) -> config.  `p` from Flux.destructure is accepted as is.
function config_for(dims::Vector{Int}, acts::Vector{Int}; time_dep, max_batch, reltol, abstol, regularize,
                    max_attempts = 160, device = 0, pre_act = false, track = true)
    d = ntuple(i -> Int32(i <= length(dims) ? dims[i] : 0), 9)
    a = ntuple(i -> Int32(i <= length(acts) ? acts[i] : 0), 8)
    tr = track ? 1 : 0      # track_ctrl, track_initdt (false: step sizes and times are constants of the reverse pass; what the tiled engine serves)
    NodeConfig(length(acts), d, a, time_dep, pre_act, max_batch, 0, reltol, abstol, regularize, 1, tr, tr, max_attempts, device, 0, 0, 0, 0)
end

"""
    solve_forward(h, x, p, tspan; keep_tape) -> (u, nfe, saveval)

Replaces `solve(prob, Tsit5(); sensealg, callback, kwargs...)` + `diffeqsol_to_trackedarray` + `sol.destats.nf`
(reference neural_ode.jl:131-142).  x, p: device arrays (Float32, column-major D x B / flat).
"""
function solve_forward(h::Handle, x::ROCMatrix{Float32}, p::ROCVector{Float32}, tspan; keep_tape::Bool)
    D, B = size(x)
    u = similar(x)
    nfe = Ref{Int64}(0)
    nsv = Ref{Int32}(0)
    sv = Vector{Float32}(undef, h.cfg.max_attempts + 1)
    GC.@preserve x p u sv begin
        st = ccall((:rnde_node_forward, LIB), Cint,
                   (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int32, Float32, Float32, Ptr{Cvoid}, Ref{Int64},
                    Ptr{Float32}, Ref{Int32}, Int32, Ptr{Cvoid}),
                   h.ptr, devptr(x), devptr(p), B, Float32(tspan[1]), Float32(tspan[2]), devptr(u), nfe,
                   sv, nsv, keep_tape ? 1 : 0, _stream())
        check(h, st)
    end
    return u, Int(nfe[]), sv[1:nsv[]]
end

"""
    solve_forward_saveat(h, x, p, tspan, saveat; keep_tape) -> (u3, nfe, saveval)

The {R,true} call methods (reference neural_ode.jl:79-108, :146-180): `u3` is the D x T x B array
`diffeqsol_to_3dtrackedarray` builds (src/utils.jl:17-19), T = length(saveat).
"""
function solve_forward_saveat(h::Handle, x::ROCMatrix{Float32}, p::ROCVector{Float32}, tspan, saveat::Vector{Float32};
                              keep_tape::Bool)
    D, B = size(x)
    u3 = ROCArray{Float32}(undef, D, length(saveat), B)
    nfe = Ref{Int64}(0)
    nsv = Ref{Int32}(0)
    sv = Vector{Float32}(undef, h.cfg.max_attempts + 1)
    GC.@preserve x p u3 sv saveat begin
        st = ccall((:rnde_node_forward_saveat, LIB), Cint,
                   (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int32, Float32, Float32, Ptr{Float32}, Int32, Ptr{Cvoid},
                    Ref{Int64}, Ptr{Float32}, Ref{Int32}, Int32, Ptr{Cvoid}),
                   h.ptr, devptr(x), devptr(p), B, Float32(tspan[1]), Float32(tspan[2]), saveat, length(saveat),
                   devptr(u3), nfe, sv, nsv, keep_tape ? 1 : 0, _stream())
        check(h, st)
    end
    return u3, Int(nfe[]), sv[1:nsv[]]
end

# save_everystep = true (neural_ode.jl:10-11): the state after every accepted step (the initial one first when save_start), D x n x B with n
# known after the call (the library solves twice: the step sequence, then the same solve saving at those step ends); backward as after saveat
function solve_forward_everystep(h::Handle, x::ROCMatrix{Float32}, p::ROCVector{Float32}, tspan; save_start::Bool = true, keep_tape::Bool)
    D, B = size(x)
    cap = h.cfg.max_attempts + 1
    buf = ROCArray{Float32}(undef, D * cap * B)
    ts = Vector{Float32}(undef, cap)
    n = Ref{Int32}(0)
    nfe = Ref{Int64}(0)
    nsv = Ref{Int32}(0)
    sv = Vector{Float32}(undef, h.cfg.max_attempts + 1)
    GC.@preserve x p buf sv ts begin
        st = ccall((:rnde_node_forward_everystep, LIB), Cint,
                   (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int32, Float32, Float32, Int32, Ptr{Cvoid}, Int32, Ptr{Float32}, Ref{Int32},
                    Ref{Int64}, Ptr{Float32}, Ref{Int32}, Int32, Ptr{Cvoid}),
                   h.ptr, devptr(x), devptr(p), B, Float32(tspan[1]), Float32(tspan[2]), save_start ? 1 : 0, devptr(buf), cap, ts, n,
                   nfe, sv, nsv, keep_tape ? 1 : 0, _stream())
        check(h, st)
    end
    u3 = reshape(buf[1:D * Int(n[]) * B], D, Int(n[]), B)
    return u3, ts[1:n[]], Int(nfe[]), sv[1:nsv[]]
end

# ubar: D x B after solve_forward, D x T x B after solve_forward_saveat; x-bar is D x B either way
function solve_backward(h::Handle, ubar::ROCArray{Float32}, svbar::Vector{Float32}, np::Int)
    xbar = ROCArray{Float32}(undef, size(ubar, 1), size(ubar, ndims(ubar)))
    pbar = ROCArray{Float32}(undef, np)
    tsbar = zeros(Float32, 2)
    GC.@preserve ubar xbar pbar svbar tsbar begin
        st = ccall((:rnde_node_backward, LIB), Cint,
                   (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float32}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float32}, Ptr{Cvoid}),
                   h.ptr, devptr(ubar), svbar, devptr(xbar), devptr(pbar), tsbar, _stream())
        check(h, st)
    end
    return xbar, pbar, tsbar
end

# ---- Tracker glue: one tape node for the whole solve ------------------------------------------------
# rnde_solve(h, x, p, tspan) returns (u, saveval); nfe is kept on the handle (non-differentiable).
rnde_solve(h::Handle, x::TrackedArray, p::TrackedArray, tspan) = track(rnde_solve, h, x, p, tspan)

@grad function rnde_solve(h::Handle, x, p, tspan)
    u, nfe, sv = solve_forward(h, data(x), data(p), data.(tspan); keep_tape = true)
    h.last_nfe = nfe
    return (u, sv), function (Δ)
        ubar, svbar = Δ
        xbar, pbar, tsbar = solve_backward(h, ROCArray{Float32}(ubar), Vector{Float32}(svbar), length(p))
        return (nothing, xbar, pbar, tsbar)
    end
end

# the {R,true} methods (reference neural_ode.jl:79-108, :146-180): u3 is D x T x B, its cotangent has the same shape
rnde_solve_saveat(h::Handle, x::TrackedArray, p::TrackedArray, tspan, saveat::Vector{Float32}) = track(rnde_solve_saveat, h, x, p, tspan, saveat)

@grad function rnde_solve_saveat(h::Handle, x, p, tspan, saveat)
    u3, nfe, sv = solve_forward_saveat(h, data(x), data(p), data.(tspan), saveat; keep_tape = true)
    h.last_nfe = nfe
    return (u3, sv), function (Δ)
        ubar, svbar = Δ
        xbar, pbar, tsbar = solve_backward(h, ROCArray{Float32}(ubar), Vector{Float32}(svbar), length(p))
        return (nothing, xbar, pbar, tsbar, nothing)
    end
end

# The unregularised methods ({false,false} / {false,true}) go through the same two rules: their handle is created with regularize = 0, the
# saved-value vector then comes back empty and its cotangent is ignored.

# ---- what changes in src/models/neural_ode.jl: bindings/julia/patch_neural_ode.jl holds the four call methods as real method
# definitions (include it after `using RegNeuralDE`); the body between ODEProblem construction and result unpacking (reference
# :126-138) is the one call below, everything else -- signature, keyword defaults, `_convert_tspan`, the returned triple -- is the reference's:
#
#
#   @fastmath function (n::TrackedNeuralODE{true,false})(x, p = n.p; func = ..., tspan = nothing, saveat = nothing)
#       tspan = _convert_tspan(isnothing(tspan) ? n.tspan : tspan, p)
#       res, saveval = RNDE.rnde_solve(n.rnde_handle, x, p, tspan)        # <- replaces :126-138
#       sv = SavedValues(eltype(tspan), eltype(p)); append!(sv.saveval, saveval)
#       return res, n.rnde_handle.last_nfe, sv
#   end
#
# and the constructor (:10-33) creates `rnde_handle = RNDE.Handle(RNDE.config_for(...))` from the Dense sizes
# of `model`, kwargs[:reltol], kwargs[:abstol] and `regularize`.

# ---- TrackedNeuralDSDE (reference src/models/neural_sde.jl) -----------------------------------------
struct NsdeConfig   # mirrors rnde_nsde_config
    drift_layers::Int32
    drift_dims::NTuple{9,Int32}
    drift_act::NTuple{8,Int32}
    diff_layers::Int32
    diff_dims::NTuple{9,Int32}
    diff_act::NTuple{8,Int32}
    max_batch::Int32
    solver::Int32          # 0 SOSRI, 1 SRIW1, 2 SOSRI2
    reltol::Float32
    abstol::Float32
    regularize::Int32
    cb_save_start::Int32
    max_attempts::Int32
    device::Int32
    beta1::Float32; beta2::Float32; gamma::Float32; qmin::Float32; qmax::Float32; qoldinit::Float32; delta::Float32
    generic::Int32
    stability_size::Float32      # RNDE_REG_STIFF: 0 = alg_stability_size(SOSRI2()) = 10.6
end

# The activation of a Dense layer (include/rnde.h: rnde_act), recognised by identity (===) with NNlib's functions as Flux re-exports them:
# Dense(in, out, relu) holds `relu` itself.  A closure such as `x -> elu(x, 0.5)` or an activation whose derivative needs the pre-activation
# (swish, gelu) is refused -- a layer that ran another map would integrate another vector field.  Shared by patch_neural_ode.jl and patch_neural_sde.jl.
const ACT_IDENTITY, ACT_TANH, ACT_RELU, ACT_SIGMOID, ACT_SOFTPLUS, ACT_ELU = Int32(0), Int32(1), Int32(2), Int32(3), Int32(4), Int32(5)
function act_code(f)
    f === identity && return ACT_IDENTITY
    f === tanh && return ACT_TANH
    f === Flux.relu && return ACT_RELU
    f === Flux.σ && return ACT_SIGMOID
    f === Flux.softplus && return ACT_SOFTPLUS
    f === Flux.elu && return ACT_ELU
    error("RNDE: Dense activation ", f, " is not served (identity, tanh, relu, σ, softplus, elu)")
end

# The leading element-wise map of a dynamics chain (include/rnde.h: rnde_pre_act): `x -> tanh.(x)` (experiments/latent_ode.jl:114) or `x -> x .^ 3`
# (experiments/sde_toy_problem.jl:45), recognised by its values at fixed points -- the rule of regneuralde_jl_amd/layers.py::pre_act_of.  Anything else is
# refused: a map the kernels do not apply must not be replaced by another one silently.
const PRE_NONE, PRE_TANH, PRE_CUBE = Int32(0), Int32(1), Int32(2)
# Same probes, same test as the Python rule: Float64 points, each value within 1e-9 relative (of max(1, |want|)) of the map's value there.
const _PRE_PROBES = Float64[-1.5, -0.3, 0.0, 0.7, 2.0]
_pre_match(v, want) = all(abs(Float64(a) - b) <= 1e-9 * max(1.0, abs(b)) for (a, b) in zip(v, want))
function pre_act_code(l)
    v = try l(_PRE_PROBES) catch; nothing end
    v isa AbstractVector && length(v) == length(_PRE_PROBES) || error("RNDE: the leading element of the chain is not an element-wise map; got ", l)
    _pre_match(v, tanh.(_PRE_PROBES)) && return PRE_TANH
    _pre_match(v, _PRE_PROBES .^ 3) && return PRE_CUBE
    error("RNDE: the leading element of the chain is neither tanh nor x -> x .^ 3 (the maps the kernels apply); got ", l)
end

mutable struct NsdeHandle
    ptr::Ptr{Cvoid}
    cfg::NsdeConfig
    function NsdeHandle(cfg::NsdeConfig)
        out = Ref{Ptr{Cvoid}}(C_NULL)
        st = ccall((:rnde_nsde_create, LIB), Cint, (Ref{NsdeConfig}, Ref{Ptr{Cvoid}}), cfg, out)
        st == 0 || error("rnde_nsde_create: ", unsafe_string(ccall((:rnde_nsde_last_error, LIB), Cstring, (Ptr{Cvoid},), C_NULL)))
        h = new(out[], cfg)
        finalizer(h -> ccall((:rnde_nsde_destroy, LIB), Cvoid, (Ptr{Cvoid},), h.ptr), h)
        return h
    end
end

"""
    nsde_forward(h, x, p, tspan; noise = nothing, seed = 0, keep_tape) -> (u, nfe1, nfe2, saveval)

Replaces `solve(prob, SOSRI(); sensealg, callback, kwargs...)` and the unpacking at neural_sde.jl:98-113.
`noise`: a `ROCArray{Float32,4}` of size (D, B, 2, n_pool) filled by `randn!` (the caller's own random stream: memory order
D fastest, then B, then W/Z, then the draw -- exactly the pool layout of include/rnde.h), or `nothing` for the library's
Philox stream named by `seed`.
"""
function nsde_forward(h::NsdeHandle, x::ROCMatrix{Float32}, p::ROCVector{Float32}, tspan; noise = nothing, seed::Integer = 0, keep_tape::Bool)
    D, B = size(x)
    u = similar(x)
    nfe1 = Ref{Int64}(0); nfe2 = Ref{Int64}(0); nsv = Ref{Int32}(0)
    sv = Vector{Float32}(undef, h.cfg.max_attempts + 1)
    npool = noise === nothing ? 0 : size(noise, 4)
    GC.@preserve x p u sv noise begin
        st = ccall((:rnde_nsde_forward, LIB), Cint,
                   (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int32, Float32, Float32, Ptr{Cvoid}, Int32, UInt64, Ptr{Cvoid},
                    Ref{Int64}, Ref{Int64}, Ptr{Float32}, Ref{Int32}, Int32, Ptr{Cvoid}),
                   h.ptr, devptr(x), devptr(p), B, Float32(tspan[1]), Float32(tspan[2]),
                   noise === nothing ? C_NULL : devptr(noise), npool, UInt64(seed), devptr(u), nfe1, nfe2, sv, nsv, keep_tape ? 1 : 0, _stream())
        st == 0 || error("rnde_nsde_forward status $st: ", unsafe_string(ccall((:rnde_nsde_last_error, LIB), Cstring, (Ptr{Cvoid},), h.ptr)))
    end
    return u, Int(nfe1[]), Int(nfe2[]), sv[1:nsv[]]
end

function nsde_backward(h::NsdeHandle, ubar::ROCMatrix{Float32}, svbar::Vector{Float32}, np::Int)
    xbar = similar(ubar)
    pbar = ROCArray{Float32}(undef, np)
    GC.@preserve ubar xbar pbar svbar begin
        st = ccall((:rnde_nsde_backward, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float32}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                   h.ptr, devptr(ubar), svbar, devptr(xbar), devptr(pbar), _stream())
        st == 0 || error("rnde_nsde_backward status $st")
    end
    return xbar, pbar
end

function nsde_forward_saveat(h::NsdeHandle, x::ROCMatrix{Float32}, p::ROCVector{Float32}, tspan, saveat::Vector{Float32}; noise = nothing,
                             seed::Integer = 0, keep_tape::Bool)
    D, B = size(x)
    u3 = ROCArray{Float32}(undef, D, length(saveat), B)
    nfe1 = Ref{Int64}(0); nfe2 = Ref{Int64}(0); nsv = Ref{Int32}(0)
    sv = Vector{Float32}(undef, h.cfg.max_attempts + 1)
    npool = noise === nothing ? 0 : size(noise, 4)
    GC.@preserve x p u3 sv noise saveat begin
        st = ccall((:rnde_nsde_forward_saveat, LIB), Cint,
                   (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int32, Float32, Float32, Ptr{Cvoid}, Int32, UInt64, Ptr{Float32}, Int32, Ptr{Cvoid},
                    Ref{Int64}, Ref{Int64}, Ptr{Float32}, Ref{Int32}, Int32, Ptr{Cvoid}),
                   h.ptr, devptr(x), devptr(p), B, Float32(tspan[1]), Float32(tspan[2]),
                   noise === nothing ? C_NULL : devptr(noise), npool, UInt64(seed), saveat, length(saveat), devptr(u3), nfe1, nfe2, sv, nsv,
                   keep_tape ? 1 : 0, _stream())
        st == 0 || error("rnde_nsde_forward_saveat status $st: ", unsafe_string(ccall((:rnde_nsde_last_error, LIB), Cstring, (Ptr{Cvoid},), h.ptr)))
    end
    return u3, Int(nfe1[]), Int(nfe2[]), sv[1:nsv[]]
end

# save_everystep = true of the SDE layer (neural_sde.jl:14): every accepted step's end (t0 first when save_start), two solves on the same noise inside
function nsde_forward_everystep(h::NsdeHandle, x::ROCMatrix{Float32}, p::ROCVector{Float32}, tspan; noise = nothing, seed::Integer = 0,
                                save_start::Bool = true, keep_tape::Bool)
    D, B = size(x)
    cap = h.cfg.max_attempts + 1
    buf = ROCArray{Float32}(undef, D * cap * B)
    ts = Vector{Float32}(undef, cap)
    n = Ref{Int32}(0); nfe1 = Ref{Int64}(0); nfe2 = Ref{Int64}(0); nsv = Ref{Int32}(0)
    sv = Vector{Float32}(undef, h.cfg.max_attempts + 1)
    npool = noise === nothing ? 0 : size(noise, 4)
    GC.@preserve x p buf sv noise ts begin
        st = ccall((:rnde_nsde_forward_everystep, LIB), Cint,
                   (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int32, Float32, Float32, Ptr{Cvoid}, Int32, UInt64, Int32, Ptr{Cvoid}, Int32, Ptr{Float32},
                    Ref{Int32}, Ref{Int64}, Ref{Int64}, Ptr{Float32}, Ref{Int32}, Int32, Ptr{Cvoid}),
                   h.ptr, devptr(x), devptr(p), B, Float32(tspan[1]), Float32(tspan[2]),
                   noise === nothing ? C_NULL : devptr(noise), npool, UInt64(seed), save_start ? 1 : 0, devptr(buf), cap, ts, n, nfe1, nfe2, sv, nsv,
                   keep_tape ? 1 : 0, _stream())
        st == 0 || error("rnde_nsde_forward_everystep status $st: ", unsafe_string(ccall((:rnde_nsde_last_error, LIB), Cstring, (Ptr{Cvoid},), h.ptr)))
    end
    return reshape(buf[1:D * Int(n[]) * B], D, Int(n[]), B), ts[1:n[]], Int(nfe1[]), Int(nfe2[]), sv[1:nsv[]]
end

# u-bar: D x B after nsde_forward, D x T x B after nsde_forward_saveat; x-bar is D x B either way
function nsde_backward_any(h::NsdeHandle, ubar::ROCArray{Float32}, svbar::Vector{Float32}, np::Int)
    xbar = ROCArray{Float32}(undef, size(ubar, 1), size(ubar, ndims(ubar)))
    pbar = ROCArray{Float32}(undef, np)
    GC.@preserve ubar xbar pbar svbar begin
        st = ccall((:rnde_nsde_backward, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float32}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                   h.ptr, devptr(ubar), svbar, devptr(xbar), devptr(pbar), _stream())
        st == 0 || error("rnde_nsde_backward status $st: ", unsafe_string(ccall((:rnde_nsde_last_error, LIB), Cstring, (Ptr{Cvoid},), h.ptr)))
    end
    return xbar, pbar
end

# Tracker glue for the stochastic layer: one tape node for the whole solve.  The evaluation counters the reference keeps in the layer's mutable
# `nfes` vector (neural_sde.jl:11, :46, :50, :142-143) are kept on the handle.  `seed` names the library's Philox stream (a caller that wants
# Julia's own random stream passes a pool of normals through nsde_forward directly).
mutable struct NsdeCounters; nfe1::Int; nfe2::Int; end
const NSDE_COUNTERS = IdDict{NsdeHandle,NsdeCounters}()
counters(h::NsdeHandle) = get!(() -> NsdeCounters(0, 0), NSDE_COUNTERS, h)

rnde_nsde_solve(h::NsdeHandle, x::TrackedArray, p::TrackedArray, tspan, seed::Integer) = track(rnde_nsde_solve, h, x, p, tspan, seed)
@grad function rnde_nsde_solve(h::NsdeHandle, x, p, tspan, seed)
    u, nfe1, nfe2, sv = nsde_forward(h, data(x), data(p), data.(tspan); seed = seed, keep_tape = true)
    c = counters(h); c.nfe1 = nfe1; c.nfe2 = nfe2
    return (u, sv), function (Δ)
        ubar, svbar = Δ
        xbar, pbar = nsde_backward_any(h, ROCArray{Float32}(ubar), Vector{Float32}(svbar), length(p))
        return (nothing, xbar, pbar, nothing, nothing)      # (the SDE step-size controller strips tracking: no tspan cotangent, DESIGN.md 4.3)
    end
end

rnde_nsde_solve_saveat(h::NsdeHandle, x::TrackedArray, p::TrackedArray, tspan, saveat::Vector{Float32}, seed::Integer) =
    track(rnde_nsde_solve_saveat, h, x, p, tspan, saveat, seed)
@grad function rnde_nsde_solve_saveat(h::NsdeHandle, x, p, tspan, saveat, seed)
    u3, nfe1, nfe2, sv = nsde_forward_saveat(h, data(x), data(p), data.(tspan), saveat; seed = seed, keep_tape = true)
    c = counters(h); c.nfe1 = nfe1; c.nfe2 = nfe2
    return (u3, sv), function (Δ)
        ubar, svbar = Δ
        xbar, pbar = nsde_backward_any(h, ROCArray{Float32}(ubar), Vector{Float32}(svbar), length(p))
        return (nothing, xbar, pbar, nothing, nothing, nothing)
    end
end

# config from the two Flux chains of TrackedNeuralDSDE (neural_sde.jl:13-41): Dense sizes and activations, tolerances from kwargs
# the chains' leading element-wise maps (PRE_NONE / PRE_TANH / PRE_CUBE) of a handle that holds no tape
function nsde_set_pre_act!(h::NsdeHandle, drift_pre::Integer, diff_pre::Integer)
    st = ccall((:rnde_nsde_set_pre_act, LIB), Cint, (Ptr{Cvoid}, Int32, Int32), h.ptr, drift_pre, diff_pre)
    st == 0 || error("rnde_nsde_set_pre_act status $st: ", unsafe_string(ccall((:rnde_nsde_last_error, LIB), Cstring, (Ptr{Cvoid},), h.ptr)))
    return h
end

function nsde_config_for(drift_dims::Vector{Int}, drift_acts::Vector{Int}, diff_dims::Vector{Int}, diff_acts::Vector{Int}; max_batch, reltol, abstol,
                         regularize, solver = 0, max_attempts = 256, device = 0)
    t9(v) = ntuple(i -> Int32(i <= length(v) ? v[i] : 0), 9)
    t8(v) = ntuple(i -> Int32(i <= length(v) ? v[i] : 0), 8)
    NsdeConfig(length(drift_acts), t9(drift_dims), t8(drift_acts), length(diff_acts), t9(diff_dims), t8(diff_acts), max_batch, solver, reltol, abstol,
               regularize, 1, max_attempts, device, 0f0, 0f0, 0f0, 0f0, 0f0, 0f0, 0f0, 0, 0f0)
end

# ---- one training-step gradient in one call ------------------------------------------------------------
# loss_function + Tracker.gradient of experiments/mnist_node.jl:132-137, :229-233 for ClassifierNODE with preode = identity:
# forward solve (taped) -> Dense(D, C) + logitcrossentropy and their reverse -> reverse solve, with the head queued before the
# forward's host wait.  Returns (ce (1-element device array), lambda * mean(saveval), nfe); the gradients land in p2bar / p3bar
# in stream order.  comm: the handle of comm_create (C_NULL: single GPU) -- both gradients are then sum-all-reduced in place.
function classifier_grad!(p2bar::ROCVector{Float32}, p3bar::ROCVector{Float32}, h::Handle, x::ROCMatrix{Float32},
                          p2::ROCVector{Float32}, p3::ROCVector{Float32}, y::ROCMatrix{Float32}, tspan; lambda = 1f2,
                          comm::Ptr{Cvoid} = C_NULL)
    ce = ROCVector{Float32}(undef, 1)
    reg = Ref{Cfloat}(0); nfe = Ref{Int64}(0)
    st = GC.@preserve p2bar p3bar x p2 p3 y ce begin
        ccall((:rnde_node_classifier_grad, LIB), Cint,
              (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int32, Int32, Cfloat, Cfloat, Cfloat,
               Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ref{Cfloat}, Ref{Int64}, Ptr{Cvoid}, Ptr{Cvoid}),
              h.ptr, devptr(x), devptr(p2), devptr(p3), devptr(y), size(x, 2), size(y, 1), Float32(tspan[1]), Float32(tspan[2]),
              Float32(lambda), devptr(p2bar), devptr(p3bar), C_NULL, devptr(ce), reg, nfe, comm, _stream())
    end
    st == 0 || error("rnde_node_classifier_grad: ", unsafe_string(ccall((:rnde_last_error, LIB), Cstring, (Ptr{Cvoid},), h.ptr)))
    return ce, reg[], nfe[]
end

# The SDE counterpart (ClassifierNSDE around the solve, one trajectory per input): x is the SDE's initial state (the presde layer's output),
# xbar its cotangent; noise = nothing: the library's Philox stream named by `seed`, else the caller's pool (D x B x 2 x n_pool normals).
function nsde_classifier_grad!(p2bar::ROCVector{Float32}, p3bar::ROCVector{Float32}, xbar::ROCMatrix{Float32}, h::NsdeHandle,
                               x::ROCMatrix{Float32}, p2::ROCVector{Float32}, p3::ROCVector{Float32}, y::ROCMatrix{Float32}, tspan;
                               lambda = 1f1, noise = nothing, seed::Integer = 0)
    ce = ROCVector{Float32}(undef, 1)
    reg = Ref{Cfloat}(0); nfe1 = Ref{Int64}(0); nfe2 = Ref{Int64}(0)
    npool = noise === nothing ? 0 : size(noise, 4)
    st = GC.@preserve p2bar p3bar xbar x p2 p3 y ce noise begin
        ccall((:rnde_nsde_classifier_grad, LIB), Cint,
              (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int32, Int32, Cfloat, Cfloat, Ptr{Cvoid}, Int32, UInt64, Cfloat,
               Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ref{Cfloat}, Ref{Int64}, Ref{Int64}, Ptr{Cvoid}),
              h.ptr, devptr(x), devptr(p2), devptr(p3), devptr(y), size(x, 2), size(y, 1), Float32(tspan[1]), Float32(tspan[2]),
              noise === nothing ? C_NULL : devptr(noise), npool, UInt64(seed), Float32(lambda),
              devptr(p2bar), devptr(p3bar), devptr(xbar), devptr(ce), reg, nfe1, nfe2, _stream())
    end
    st == 0 || error("rnde_nsde_classifier_grad: ", unsafe_string(ccall((:rnde_nsde_last_error, LIB), Cstring, (Ptr{Cvoid},), h.ptr)))
    return ce, reg[], nfe1[], nfe2[]
end

# ---- ClassifierNSDE with several trajectories per input (src/models/supervised_classification.jl:82-100) ----------------
# Column j = t * B + b of every D x (B * T) array is trajectory t of input b: what repeat(x, 1, T) gives (:92, :102-103).
_nsde_err(h::NsdeHandle, who) = error(who, ": ", unsafe_string(ccall((:rnde_nsde_last_error, LIB), Cstring, (Ptr{Cvoid},), h.ptr)))

# postsde + mean over the trajectories + logitcrossentropy and their reverse (:96-98): u, ubar are D x (B * T), y is C x B.
# Returns (ce (1-element device array), logits (C x B, averaged)); ubar and p3bar are filled in stream order.
function nsde_classifier_head_traj!(ubar::ROCMatrix{Float32}, p3bar::ROCVector{Float32}, h::NsdeHandle, u::ROCMatrix{Float32},
                                    p3::ROCVector{Float32}, y::ROCMatrix{Float32}, trajectories::Integer)
    ce = ROCVector{Float32}(undef, 1)
    logits = ROCMatrix{Float32}(undef, size(y, 1), size(y, 2))
    st = GC.@preserve ubar p3bar u p3 y ce logits begin
        ccall((:rnde_nsde_classifier_head_traj, LIB), Cint,
              (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int32, Int32, Int32, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
              h.ptr, devptr(u), devptr(p3), devptr(y), size(y, 2), trajectories, size(y, 1), devptr(logits), devptr(ubar), devptr(p3bar),
              devptr(ce), _stream())
    end
    st == 0 || _nsde_err(h, "rnde_nsde_classifier_head_traj")
    return ce, logits
end

# nsde_classifier_grad! with `trajectories` sample paths per input: x (D x B, NOT repeated) is the presde layer's output, xbar (D x B) its
# cotangent, already summed over the trajectories; noise = nothing or the caller's pool (D x (B * trajectories) x 2 x n_pool normals).
function nsde_classifier_grad_traj!(p2bar::ROCVector{Float32}, p3bar::ROCVector{Float32}, xbar::ROCMatrix{Float32}, h::NsdeHandle,
                                    x::ROCMatrix{Float32}, p2::ROCVector{Float32}, p3::ROCVector{Float32}, y::ROCMatrix{Float32}, tspan;
                                    trajectories::Integer = 10, lambda = 1f1, noise = nothing, seed::Integer = 0)
    ce = ROCVector{Float32}(undef, 1)
    reg = Ref{Cfloat}(0); nfe1 = Ref{Int64}(0); nfe2 = Ref{Int64}(0)
    npool = noise === nothing ? 0 : size(noise, 4)
    st = GC.@preserve p2bar p3bar xbar x p2 p3 y ce noise begin
        ccall((:rnde_nsde_classifier_grad_traj, LIB), Cint,
              (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int32, Int32, Int32, Cfloat, Cfloat, Ptr{Cvoid}, Int32, UInt64, Cfloat,
               Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ref{Cfloat}, Ref{Int64}, Ref{Int64}, Ptr{Cvoid}),
              h.ptr, devptr(x), devptr(p2), devptr(p3), devptr(y), size(x, 2), trajectories, size(y, 1), Float32(tspan[1]), Float32(tspan[2]),
              noise === nothing ? C_NULL : devptr(noise), npool, UInt64(seed), Float32(lambda),
              devptr(p2bar), devptr(p3bar), devptr(xbar), devptr(ce), reg, nfe1, nfe2, _stream())
    end
    st == 0 || _nsde_err(h, "rnde_nsde_classifier_grad_traj")
    return ce, reg[], nfe1[], nfe2[]
end

# The evaluation call (experiments/mnist_nsde.jl:154-155; src/metrics.jl:2-9): averaged logits (C x B) of x (D x B, the presde layer's
# output) over `trajectories` untaped sample paths; with labels y (C x B) the matches of argmax(logits) against argmax(y) are ADDED to the
# one-element device counter `correct` (zero it once per data set, read it once).  Returns (logits, nfe1, nfe2).
function nsde_classifier_predict(h::NsdeHandle, x::ROCMatrix{Float32}, p2::ROCVector{Float32}, p3::ROCVector{Float32}, n_classes::Integer, tspan;
                                 trajectories::Integer = 10, y::Union{Nothing, ROCMatrix{Float32}} = nothing,
                                 correct::Union{Nothing, ROCVector{Int64}} = nothing, noise = nothing, seed::Integer = 0)
    (y === nothing && correct !== nothing) && error("nsde_classifier_predict: a counter without labels")
    logits = ROCMatrix{Float32}(undef, n_classes, size(x, 2))
    nfe1 = Ref{Int64}(0); nfe2 = Ref{Int64}(0)
    npool = noise === nothing ? 0 : size(noise, 4)
    st = GC.@preserve x p2 p3 y correct noise logits begin
        ccall((:rnde_nsde_classifier_predict, LIB), Cint,
              (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int32, Int32, Int32, Cfloat, Cfloat, Ptr{Cvoid}, Int32, UInt64,
               Ptr{Cvoid}, Ptr{Cvoid}, Ref{Int64}, Ref{Int64}, Ptr{Cvoid}),
              h.ptr, devptr(x), devptr(p2), devptr(p3), y === nothing ? C_NULL : devptr(y), size(x, 2), trajectories, n_classes,
              Float32(tspan[1]), Float32(tspan[2]), noise === nothing ? C_NULL : devptr(noise), npool, UInt64(seed),
              devptr(logits), correct === nothing ? C_NULL : devptr(correct), nfe1, nfe2, _stream())
    end
    st == 0 || _nsde_err(h, "rnde_nsde_classifier_predict")
    return logits, nfe1[], nfe2[]
end

# The evaluation call of ClassifierNODE (experiments/mnist_node.jl:185-186, :250-251; src/metrics.jl:2-18) with preode = identity: the untaped
# solve of x (D x B), the logits (C x B) of the post-layer p3 on its end state and, with labels y (C x B), the matches of argmax(logits)
# against argmax(y) ADDED to the one-element device counter `correct` (zero it once per data set, read it once).  Returns (logits, nfe).
function classifier_predict(h::Handle, x::ROCMatrix{Float32}, p2::ROCVector{Float32}, p3::ROCVector{Float32}, n_classes::Integer, tspan;
                            y::Union{Nothing, ROCMatrix{Float32}} = nothing, correct::Union{Nothing, ROCVector{Int64}} = nothing)
    (y === nothing && correct !== nothing) && error("classifier_predict: a counter without labels")
    logits = ROCMatrix{Float32}(undef, n_classes, size(x, 2))
    nfe = Ref{Int64}(0)
    st = GC.@preserve x p2 p3 y correct logits begin
        ccall((:rnde_node_classifier_predict, LIB), Cint,
              (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int32, Int32, Cfloat, Cfloat, Ptr{Cvoid}, Ptr{Cvoid}, Ref{Int64}, Ptr{Cvoid}),
              h.ptr, devptr(x), devptr(p2), devptr(p3), y === nothing ? C_NULL : devptr(y), size(x, 2), n_classes,
              Float32(tspan[1]), Float32(tspan[2]), devptr(logits), correct === nothing ? C_NULL : devptr(correct), nfe, _stream())
    end
    st == 0 || error("rnde_node_classifier_predict: ", unsafe_string(ccall((:rnde_last_error, LIB), Cstring, (Ptr{Cvoid},), h.ptr)))
    return logits, nfe[]
end

# One batch of total_loss_on_dataset (experiments/latent_ode.jl:271-292) behind the layer call: gen_to_data (p4) on the saved states res
# (20 x T x B) and sum((pred .* m .- d .* m) .^ 2) ./ sum(m) per sample against x = vcat(d, m, _t) (75 x T x B).  `lat` is the rnde_latent*
# of rnde_latent_create (this module wraps no latent handle: the pointer is passed as it is).  acc_sum (1 Float64) and acc_count (1 Int64):
# the data set's running sum and count on the device, both or neither.  Returns the B per-sample values.
function latent_decode_mse(lat::Ptr{Cvoid}, res::ROCArray{Float32, 3}, p4::ROCVector{Float32}, x::ROCArray{Float32, 3};
                           acc_sum::Union{Nothing, ROCVector{Float64}} = nothing, acc_count::Union{Nothing, ROCVector{Int64}} = nothing)
    ((acc_sum === nothing) != (acc_count === nothing)) && error("latent_decode_mse: acc_sum and acc_count go together")
    mse = ROCVector{Float32}(undef, size(res, 3))
    st = GC.@preserve res p4 x acc_sum acc_count mse begin
        ccall((:rnde_latent_decode_mse, LIB), Cint,
              (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int32, Int32, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
              lat, devptr(res), devptr(p4), devptr(x), size(res, 3), size(res, 2), devptr(mse),
              acc_sum === nothing ? C_NULL : devptr(acc_sum), acc_count === nothing ? C_NULL : devptr(acc_count), _stream())
    end
    st == 0 || error("rnde_latent_decode_mse: ", unsafe_string(ccall((:rnde_latent_last_error, LIB), Cstring, (Ptr{Cvoid},), lat)))
    return mse
end

# ---- optimiser step and the data-parallel collective -------------------------------------------------
# Optimiser(InvDecay(gamma), Momentum(eta, rho)) on one flat group, in place (src/utils.jl:149-156, mnist_node.jl:130);
# `n` is the group's InvDecay counter (starts at 1, the caller increments it); gscale = 1 / nworkers after a summed all-reduce.
function momentum_step!(p::ROCVector{Float32}, g::ROCVector{Float32}, v::ROCVector{Float32}, n::Integer;
                        gamma = 1f-5, eta = 0.1f0, rho = 0.9f0, gscale = 1f0)
    GC.@preserve p g v begin
        st = ccall((:rnde_momentum_step_scaled, LIB), Cint,
                   (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Cfloat, Cfloat, Cfloat, Cfloat, Ptr{Cvoid}),
                   devptr(p), devptr(g), devptr(v), length(p), n, gamma, eta, rho, gscale, _stream())
    end
    st == 0 || error("rnde_momentum_step_scaled: status $st")
    return p
end

# Flux.Optimise.ADAM(eta, (beta1, beta2)) on one flat parameter group (experiments/mnist_nsde.jl): m, v are the caller's state arrays (zeros at t = 1)
function adam_step!(p::ROCVector{Float32}, g::ROCVector{Float32}, m::ROCVector{Float32}, v::ROCVector{Float32}, t::Integer;
                    eta = 0.001f0, beta = (0.9f0, 0.999f0), eps = 1f-8, gscale = 1f0)
    st = GC.@preserve p g m v begin
        ccall((:rnde_adam_step, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Cfloat, Cfloat, Cfloat, Cfloat, Cfloat, Ptr{Cvoid}),
              devptr(p), devptr(g), devptr(m), devptr(v), length(p), t, eta, beta[1], beta[2], eps, gscale, _stream())
    end
    st == 0 || error("rnde_adam_step: status $st")
    return p
end

# Flux.Optimise.Optimiser(WeightDecay(wd), ADAM(eta, (beta1, beta2))) on one flat group, one launch (experiments/ffjord_gaussian.jl:132,
# ffjord_tabular.jl:133): g' = gscale * g + wd * p, then adam_step!'s recurrence
function adam_wd_step!(p::ROCVector{Float32}, g::ROCVector{Float32}, m::ROCVector{Float32}, v::ROCVector{Float32}, t::Integer;
                       eta = 0.001f0, beta = (0.9f0, 0.999f0), eps = 1f-8, gscale = 1f0, wd = 1f-5)
    st = GC.@preserve p g m v begin
        ccall((:rnde_adam_wd_step, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Cfloat, Cfloat, Cfloat, Cfloat, Cfloat, Cfloat, Ptr{Cvoid}),
              devptr(p), devptr(g), devptr(m), devptr(v), length(p), t, eta, beta[1], beta[2], eps, gscale, wd, _stream())
    end
    st == 0 || error("rnde_adam_wd_step: status $st")
    return p
end

# one process per GPU (Distributed / MPI.jl carry the 128-byte id from rank 0 to the others)
comm_unique_id() = (id = zeros(UInt8, 128); ccall((:rnde_comm_unique_id, LIB), Cint, (Ptr{UInt8},), id) == 0 || error("rnde_comm_unique_id"); id)
function comm_create(id::Vector{UInt8}, rank::Integer, world::Integer, device::Integer)
    out = Ref{Ptr{Cvoid}}(C_NULL)
    ccall((:rnde_comm_create, LIB), Cint, (Ptr{UInt8}, Int32, Int32, Int32, Ref{Ptr{Cvoid}}), id, rank, world, device, out) == 0 ||
        error("rnde_comm_create: ", unsafe_string(ccall((:rnde_comm_last_error, LIB), Cstring, (Ptr{Cvoid},), C_NULL)))
    return out[]
end
allreduce_sum!(comm::Ptr{Cvoid}, g::ROCVector{Float32}) = GC.@preserve g begin
    ccall((:rnde_comm_allreduce, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int32, Ptr{Cvoid}), comm, devptr(g), length(g), 0, _stream()) == 0 ||
        error("rnde_comm_allreduce")
    g
end

# The same all-reduce as ONE kernel over peer-mapped windows (opt-in, include/rnde.h): every rank makes a window, the 64-byte handles travel to
# all ranks in rank order (Distributed / MPI.jl: an all-gather of 64 bytes), comm_create_peers maps them.  `ENV["RNDE_ONESHOT"] = "1"` in front of
# comm_create does the same through RCCL's own all-gather.  comm_path says which path a communicator's all-reduces take.
function comm_window_create(device::Integer)
    win = Ref{Ptr{Cvoid}}(C_NULL); handle = zeros(UInt8, 64)
    ccall((:rnde_comm_window_create, LIB), Cint, (Int32, Ref{Ptr{Cvoid}}, Ptr{UInt8}), device, win, handle) == 0 ||
        error("rnde_comm_window_create: ", unsafe_string(ccall((:rnde_comm_last_error, LIB), Cstring, (Ptr{Cvoid},), C_NULL)))
    return win[], handle
end
function comm_create_peers(win::Ptr{Cvoid}, handles::Vector{UInt8}, rank::Integer, world::Integer)
    length(handles) == 64 * world || error("comm_create_peers: 64 bytes per rank, in rank order")
    out = Ref{Ptr{Cvoid}}(C_NULL)
    ccall((:rnde_comm_create_peers, LIB), Cint, (Ptr{Cvoid}, Ptr{UInt8}, Int32, Int32, Ref{Ptr{Cvoid}}), win, handles, rank, world, out) == 0 ||
        error("rnde_comm_create_peers: ", unsafe_string(ccall((:rnde_comm_last_error, LIB), Cstring, (Ptr{Cvoid},), C_NULL)))
    return out[]
end
comm_path(comm::Ptr{Cvoid}) = unsafe_string(ccall((:rnde_comm_path, LIB), Cstring, (Ptr{Cvoid},), comm))

# SURVEY 8e mode 2: ONE step-size controller for all column shards of a minibatch (rnde_node_set_coupling): every rank calls it with
# its communicator and the global batch; `comm = C_NULL` returns to independent controllers.  Equal shards, the same calls on every rank.
function set_coupling!(h::Handle, comm::Ptr{Cvoid}, global_batch::Integer)
    st = ccall((:rnde_node_set_coupling, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int32), h.ptr, comm, global_batch)
    st == 0 || error("rnde_node_set_coupling: ", unsafe_string(ccall((:rnde_last_error, LIB), Cstring, (Ptr{Cvoid},), h.ptr)))
    return h
end

# Which unit forms the Dense-layer products of the one-launch forward solve (include/rnde.h: rnde_node_set_matrix_mode):
# 0 = fp32-input MFMA (vector ALUs on gfx950), 1 = exact three-way bf16 split on the matrix cores (the default where the kernels serve the shape).
function set_matrix_mode!(h::Handle, mode::Integer)
    st = ccall((:rnde_node_set_matrix_mode, LIB), Cint, (Ptr{Cvoid}, Cint), h.ptr, Cint(mode))
    check(h, st)
end
matrix_mode(h::Handle) = Int(ccall((:rnde_node_matrix_mode, LIB), Cint, (Ptr{Cvoid},), h.ptr))

# ---- TrackedFFJORD with the ConcatSquash MLPDynamics (include/rnde.h, "TrackedFFJORD") ----
struct FfjordConfig
    in_dims::Int32; hidden::Int32; dynamics::Int32; time_dep::Int32; regularize::Int32; kinetic_reg::Int32
    max_batch::Int32; solver::Int32; reltol::Float32; abstol::Float32; cb_save_start::Int32; max_attempts::Int32; device::Int32
end
# the default dynamics (Tracker.forward through a Dense chain, then back): rnde_ffjord_chain_config, served by rnde_ffjord_create_chain
struct FfjordChainConfig
    n_layers::Int32
    dims::NTuple{9,Int32}
    act::NTuple{8,Int32}
    time_dep::Int32; regularize::Int32; max_batch::Int32; solver::Int32; reltol::Float32; abstol::Float32
    cb_save_start::Int32; max_attempts::Int32; device::Int32
end
function ffjord_chain_config(dims::Vector{Int}, acts::Vector{Int}; time_dep, regularize, max_batch, reltol, abstol, max_attempts = 4096, device = 0)
    d = ntuple(i -> Int32(i <= length(dims) ? dims[i] : 0), 9)
    a = ntuple(i -> Int32(i <= length(acts) ? acts[i] : 0), 8)
    FfjordChainConfig(length(acts), d, a, time_dep, regularize, max_batch, 0, reltol, abstol, 1, max_attempts, device)
end
ffjord_chain_param_count(cfg::FfjordChainConfig) = Int(ccall((:rnde_ffjord_chain_param_count, LIB), Int32, (Ref{FfjordChainConfig},), cfg))
ffjord_engine(h) = Int(ccall((:rnde_ffjord_engine, LIB), Int32, (Ptr{Cvoid},), h.ptr))     # 0: one workgroup, 1: tiled, 2: chain dynamics
# the tracked-controller reverse sweep (engines 1 and 2, regularize = 1 handles, no tape held): ffjord_backward then differentiates the PI
# controller as well (track_ctrl = 1, track_initdt = 0); the tape remembers the setting of its forward
function ffjord_set_track_ctrl(h, on::Bool)
    st = ccall((:rnde_ffjord_set_track_ctrl, LIB), Cint, (Ptr{Cvoid}, Int32), h.ptr, Int32(on))
    st == 0 || error("rnde_ffjord_set_track_ctrl status $st: ", _fferr(h.ptr))
    return on
end
ffjord_track_ctrl(h) = Int(ccall((:rnde_ffjord_track_ctrl, LIB), Int32, (Ptr{Cvoid},), h.ptr)) == 1
ffjord_param_count(cfg::FfjordConfig) = Int(ccall((:rnde_ffjord_param_count, LIB), Int32, (Ref{FfjordConfig},), cfg))
_fferr(p) = unsafe_string(ccall((:rnde_ffjord_last_error, LIB), Cstring, (Ptr{Cvoid},), p))

mutable struct FfjordHandle
    ptr::Ptr{Cvoid}
    cfg::Union{FfjordConfig,FfjordChainConfig}
    # engine = :workgroup (rnde_ffjord_create: in + 1 <= 64, h <= 64) or :tiled (rnde_ffjord_create_tiled: in <= 64, h <= 112), as Python's engine=
    function FfjordHandle(cfg::FfjordConfig; engine::Symbol = :workgroup)
        out = Ref{Ptr{Cvoid}}(C_NULL)
        if engine === :tiled
            st = ccall((:rnde_ffjord_create_tiled, LIB), Cint, (Ref{FfjordConfig}, Ref{Ptr{Cvoid}}), cfg, out)
        elseif engine === :workgroup
            st = ccall((:rnde_ffjord_create, LIB), Cint, (Ref{FfjordConfig}, Ref{Ptr{Cvoid}}), cfg, out)
        else
            error("RNDE: engine must be :workgroup or :tiled; got ", engine)
        end
        st == 0 || error("rnde_ffjord_create ($engine): ", _fferr(C_NULL))
        h = new(out[], cfg)
        finalizer(h -> ccall((:rnde_ffjord_destroy, LIB), Cvoid, (Ptr{Cvoid},), h.ptr), h)
        return h
    end
    # a Dense chain under the default dynamics: one engine (the tiled layout), every other ffjord_* call dispatches on the handle
    function FfjordHandle(cfg::FfjordChainConfig)
        out = Ref{Ptr{Cvoid}}(C_NULL)
        st = ccall((:rnde_ffjord_create_chain, LIB), Cint, (Ref{FfjordChainConfig}, Ref{Ptr{Cvoid}}), cfg, out)
        st == 0 || error("rnde_ffjord_create_chain: ", _fferr(C_NULL))
        h = new(out[], cfg)
        finalizer(h -> ccall((:rnde_ffjord_destroy, LIB), Cvoid, (Ptr{Cvoid},), h.ptr), h)
        return h
    end
end

# forward: x, e (D x B) -> logpx (B), nfe, saved values (EEst * dt per accepted step, {true} only); keeps the tape for ffjord_backward
function ffjord_forward(h::FfjordHandle, x::ROCMatrix{Float32}, p::ROCVector{Float32}, e::ROCMatrix{Float32}, tspan; keep_tape::Bool = true)
    B = size(x, 2)
    logpx = similar(x, B)
    nfe = Ref{Int64}(0); nsv = Ref{Int32}(0)
    sv = Vector{Float32}(undef, h.cfg.max_attempts + 1)
    GC.@preserve x p e logpx begin
        st = ccall((:rnde_ffjord_forward, LIB), Cint,
                   (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int32, Float32, Float32, UInt64, Ptr{Cvoid}, Ptr{Cvoid}, Ref{Int64}, Ptr{Float32}, Ref{Int32}, Int32, Ptr{Cvoid}),
                   h.ptr, devptr(x), devptr(p), devptr(e), B, Float32(tspan[1]), Float32(tspan[2]), UInt64(0), devptr(logpx), C_NULL, nfe, sv, nsv,
                   keep_tape ? 1 : 0, _stream())
        st == 0 || error("rnde_ffjord_forward status $st: ", _fferr(h.ptr))
    end
    return logpx, Int(nfe[]), sv[1:nsv[]]
end

# reverse of the last taped forward: cotangents of logpx and of the saved values -> (p-bar, x-bar)
function ffjord_backward(h::FfjordHandle, logpx_bar::ROCVector{Float32}, svbar::Vector{Float32}, np::Int, D::Int)
    B = length(logpx_bar)
    pbar = similar(logpx_bar, np)
    xbar = similar(logpx_bar, D, B)
    GC.@preserve logpx_bar pbar xbar svbar begin
        st = ccall((:rnde_ffjord_backward, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float32}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                   h.ptr, devptr(logpx_bar), isempty(svbar) ? C_NULL : pointer(svbar), devptr(pbar), devptr(xbar), _stream())
        st == 0 || error("rnde_ffjord_backward status $st: ", _fferr(h.ptr))
    end
    return pbar, xbar
end

# Tracker glue: one tape node per forward, (logpx, saveval) -> (x-bar, p-bar).  A handle holds ONE tape and only a taped forward replaces it
# (untaped calls leave it alone): the node's backward must run before the next tracked call on the same handle, as Tracker.gradient does.
const FFJORD_NFE = IdDict{FfjordHandle,Int}()
ffjord_solve(h::FfjordHandle, x::TrackedArray, p::TrackedArray, e, tspan) = track(ffjord_solve, h, x, p, e, tspan)
ffjord_solve(h::FfjordHandle, x, p::TrackedArray, e, tspan) = track(ffjord_solve, h, x, p, e, tspan)
function ffjord_solve(h::FfjordHandle, x, p, e, tspan)          # nothing tracked: no tape
    logpx, nfe, sv = ffjord_forward(h, data(x), data(p), e, tspan; keep_tape = false)
    FFJORD_NFE[h] = nfe
    return logpx, sv
end
@grad function ffjord_solve(h::FfjordHandle, x, p, e, tspan)
    logpx, nfe, sv = ffjord_forward(h, data(x), data(p), e, data.(tspan); keep_tape = true)
    FFJORD_NFE[h] = nfe
    return (logpx, sv), function (Δ)
        lb, svb = Δ
        lbar = lb === nothing ? fill!(similar(logpx), 0f0) : ROCArray{Float32}(data(lb))
        svbar = svb === nothing ? Float32[] : Vector{Float32}(data(svb))
        pbar, xbar = ffjord_backward(h, lbar, svbar, length(p), size(x, 1))
        return (nothing, xbar, pbar, nothing, nothing)
    end
end

# TrackedFFJORD{false} called with regularize = true: the state [z; l; lambda1; lambda2] (kinetic energy, Jacobian norm); reg is 2 x B
function ffjord_forward_kinetic(h::FfjordHandle, x::ROCMatrix{Float32}, p::ROCVector{Float32}, e::ROCMatrix{Float32}, tspan; keep_tape::Bool = true)
    B = size(x, 2)
    logpx = similar(x, B)
    reg = similar(x, B, 2)                                 # column-major B x 2 == the library's 2 x B rows
    nfe = Ref{Int64}(0)
    GC.@preserve x p e logpx reg begin
        st = ccall((:rnde_ffjord_forward_kinetic, LIB), Cint,
                   (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int32, Float32, Float32, UInt64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ref{Int64}, Int32, Ptr{Cvoid}),
                   h.ptr, devptr(x), devptr(p), devptr(e), B, Float32(tspan[1]), Float32(tspan[2]), UInt64(0), devptr(logpx), devptr(reg), C_NULL, nfe,
                   keep_tape ? 1 : 0, _stream())
        st == 0 || error("rnde_ffjord_forward_kinetic status $st: ", _fferr(h.ptr))
    end
    return logpx, reg[:, 1], reg[:, 2], Int(nfe[])
end

function ffjord_backward_kinetic(h::FfjordHandle, logpx_bar::ROCVector{Float32}, reg_bar::ROCMatrix{Float32}, np::Int, D::Int)
    B = length(logpx_bar)
    pbar = similar(logpx_bar, np)
    xbar = similar(logpx_bar, D, B)
    GC.@preserve logpx_bar reg_bar pbar xbar begin
        st = ccall((:rnde_ffjord_backward_kinetic, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                   h.ptr, devptr(logpx_bar), devptr(reg_bar), devptr(pbar), devptr(xbar), _stream())
        st == 0 || error("rnde_ffjord_backward_kinetic status $st: ", _fferr(h.ptr))
    end
    return pbar, xbar
end

# The gradient of the experiments' loss_function in one call (rnde_ffjord_nll_grad): the taped forward, the loss terms and the sweep's
# seeds on the device, the reverse sweep.  mode 0: Hutchinson probe e (nothing: the library's draw from seed), 1: exact trace (e = nothing),
# 2: the kinetic rows.  Returns (pbar, xbar, terms, reg, nfe): terms is a 3-vector on the device, (-mean(logpx), mean(lambda1), mean(lambda2)),
# reg = lambda_r * mean(sv.saveval) on the host.  The handle holds no tape afterwards.
function ffjord_nll_grad(h::FfjordHandle, x::ROCMatrix{Float32}, p::ROCVector{Float32}, e::Union{Nothing,ROCMatrix{Float32}}, tspan;
                         mode::Integer = 0, lambda_r = 0f0, lambda_k = 0f0, lambda_j = 0f0, seed::Integer = 0, need_xbar::Bool = false)
    D, B = size(x)
    pbar = similar(p)
    xbar = need_xbar ? similar(x) : nothing
    terms = similar(p, 3)
    reg = Ref{Float32}(0f0)
    nfe = Ref{Int64}(0)
    GC.@preserve x p e pbar xbar terms begin
        st = ccall((:rnde_ffjord_nll_grad, LIB), Cint,
                   (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int32, Float32, Float32, UInt64, Int32, Float32, Float32, Float32, Ptr{Cvoid}, Ptr{Cvoid},
                    Ptr{Cvoid}, Ptr{Cvoid}, Ref{Float32}, Ref{Int64}, Ptr{Cvoid}),
                   h.ptr, devptr(x), devptr(p), e === nothing ? C_NULL : devptr(e), B, Float32(tspan[1]), Float32(tspan[2]), UInt64(seed), Int32(mode),
                   Float32(lambda_r), Float32(lambda_k), Float32(lambda_j), devptr(pbar), xbar === nothing ? C_NULL : devptr(xbar), C_NULL, devptr(terms),
                   reg, nfe, _stream())
        st == 0 || error("rnde_ffjord_nll_grad status $st: ", _fferr(h.ptr))
    end
    return pbar, xbar, terms, reg[], Int(nfe[])
end

# Tracker glue of the kinetic call: (logpx, lambda1, lambda2) -> (x-bar, p-bar); a missing cotangent counts as zeros
ffjord_solve_kinetic(h::FfjordHandle, x::TrackedArray, p::TrackedArray, e, tspan) = track(ffjord_solve_kinetic, h, x, p, e, tspan)
ffjord_solve_kinetic(h::FfjordHandle, x, p::TrackedArray, e, tspan) = track(ffjord_solve_kinetic, h, x, p, e, tspan)
function ffjord_solve_kinetic(h::FfjordHandle, x, p, e, tspan)  # nothing tracked: no tape
    logpx, l1, l2, nfe = ffjord_forward_kinetic(h, data(x), data(p), e, tspan; keep_tape = false)
    FFJORD_NFE[h] = nfe
    return logpx, l1, l2
end
@grad function ffjord_solve_kinetic(h::FfjordHandle, x, p, e, tspan)
    logpx, l1, l2, nfe = ffjord_forward_kinetic(h, data(x), data(p), e, data.(tspan); keep_tape = true)
    FFJORD_NFE[h] = nfe
    return (logpx, l1, l2), function (Δ)
        B = length(logpx)
        col(d) = d === nothing ? fill!(similar(logpx), 0f0) : ROCArray{Float32}(data(d))
        pbar, xbar = ffjord_backward_kinetic(h, col(Δ[1]), hcat(col(Δ[2]), col(Δ[3])), length(p), size(x, 1))
        return (nothing, xbar, pbar, nothing, nothing)
    end
end

# The exact-trace forward (an extension: the reference evaluates -tr J only inside sample()): no probe; engines :tiled and chain handles.
# The tape remembers that it is exact, so the reverse pass is ffjord_backward.
function ffjord_forward_exact(h::FfjordHandle, x::ROCMatrix{Float32}, p::ROCVector{Float32}, tspan; keep_tape::Bool = true)
    B = size(x, 2)
    logpx = similar(x, B)
    nfe = Ref{Int64}(0); nsv = Ref{Int32}(0)
    sv = Vector{Float32}(undef, h.cfg.max_attempts + 1)
    GC.@preserve x p logpx begin
        st = ccall((:rnde_ffjord_forward_exact, LIB), Cint,
                   (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int32, Float32, Float32, Ptr{Cvoid}, Ptr{Cvoid}, Ref{Int64}, Ptr{Float32}, Ref{Int32}, Int32, Ptr{Cvoid}),
                   h.ptr, devptr(x), devptr(p), B, Float32(tspan[1]), Float32(tspan[2]), devptr(logpx), C_NULL, nfe, sv, nsv, keep_tape ? 1 : 0, _stream())
        st == 0 || error("rnde_ffjord_forward_exact status $st: ", _fferr(h.ptr))
    end
    return logpx, Int(nfe[]), sv[1:nsv[]]
end

# the parity instrument: the exact solve along given (dt, accepted) pairs, flattened
function ffjord_forward_exact_replay(h::FfjordHandle, x::ROCMatrix{Float32}, p::ROCVector{Float32}, tspan, steps::Vector{Float32}; keep_tape::Bool = true)
    B = size(x, 2)
    logpx = similar(x, B)
    nfe = Ref{Int64}(0); nsv = Ref{Int32}(0)
    sv = Vector{Float32}(undef, h.cfg.max_attempts + 1)
    GC.@preserve x p logpx steps begin
        st = ccall((:rnde_ffjord_forward_exact_replay, LIB), Cint,
                   (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int32, Float32, Float32, Ptr{Float32}, Int32, Ptr{Cvoid}, Ptr{Cvoid}, Ref{Int64}, Ptr{Float32}, Ref{Int32}, Int32, Ptr{Cvoid}),
                   h.ptr, devptr(x), devptr(p), B, Float32(tspan[1]), Float32(tspan[2]), steps, length(steps) ÷ 2, devptr(logpx), C_NULL, nfe, sv, nsv,
                   keep_tape ? 1 : 0, _stream())
        st == 0 || error("rnde_ffjord_forward_exact_replay status $st: ", _fferr(h.ptr))
    end
    return logpx, Int(nfe[]), sv[1:nsv[]]
end

# Tracker glue of the exact call: (logpx, saveval) -> (x-bar, p-bar), as ffjord_solve without the probe
ffjord_solve_exact(h::FfjordHandle, x::TrackedArray, p::TrackedArray, tspan) = track(ffjord_solve_exact, h, x, p, tspan)
ffjord_solve_exact(h::FfjordHandle, x, p::TrackedArray, tspan) = track(ffjord_solve_exact, h, x, p, tspan)
function ffjord_solve_exact(h::FfjordHandle, x, p, tspan)       # nothing tracked: no tape
    logpx, nfe, sv = ffjord_forward_exact(h, data(x), data(p), tspan; keep_tape = false)
    FFJORD_NFE[h] = nfe
    return logpx, sv
end
@grad function ffjord_solve_exact(h::FfjordHandle, x, p, tspan)
    logpx, nfe, sv = ffjord_forward_exact(h, data(x), data(p), data.(tspan); keep_tape = true)
    FFJORD_NFE[h] = nfe
    return (logpx, sv), function (Δ)
        lb, svb = Δ
        lbar = lb === nothing ? fill!(similar(logpx), 0f0) : ROCArray{Float32}(data(lb))
        svbar = svb === nothing ? Float32[] : Vector{Float32}(data(svb))
        pbar, xbar = ffjord_backward(h, lbar, svbar, length(p), size(x, 1))
        return (nothing, xbar, pbar, nothing)
    end
end

# sample: z (D x n) solved from t1 back to t0 with the exact trace -> x (D x n)
function ffjord_sample(h::FfjordHandle, p::ROCVector{Float32}, z::ROCMatrix{Float32}, tspan)
    x = similar(z)
    GC.@preserve p z x begin
        st = ccall((:rnde_ffjord_sample, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int32, Float32, Float32, UInt64, Ptr{Cvoid}, Ptr{Cvoid}),
                   h.ptr, devptr(p), devptr(z), size(z, 2), Float32(tspan[1]), Float32(tspan[2]), UInt64(0), devptr(x), _stream())
        st == 0 || error("rnde_ffjord_sample status $st: ", _fferr(h.ptr))
    end
    return x
end

# Several batches per launch (the likelihood pass of src/metrics.jl:20-33; engines :tiled and chain handles).  The capacity is the switch:
# ffjord_reserve_groups(h, max_groups, max_columns) (0, 0 releases it); every group takes ceil(B_g / 16) tiles of its own.
function ffjord_reserve_groups(h::FfjordHandle, max_groups::Integer, max_columns::Integer)
    st = ccall((:rnde_ffjord_reserve_groups, LIB), Cint, (Ptr{Cvoid}, Int32, Int32), h.ptr, Int32(max_groups), Int32(max_columns))
    st == 0 || error("rnde_ffjord_reserve_groups status $st: ", _fferr(h.ptr))
    return nothing
end
function ffjord_group_capacity(h::FfjordHandle)
    g = Ref{Int32}(0); c = Ref{Int32}(0)
    ccall((:rnde_ffjord_group_capacity, LIB), Cint, (Ptr{Cvoid}, Ref{Int32}, Ref{Int32}), h.ptr, g, c)
    return Int(g[]), Int(c[])
end
# x, e: D x sum(Bs), the groups' columns back to back (e === nothing: the exact trace).  acc === nothing, or a ROCVector{Float64} of two
# entries: acc[1] += sum(logpx), and the second entry, read as an Int64, += sum(Bs) -- queued, not waited for.  Returns logpx (sum(Bs)), the
# NFEs and every group's status; each group bit for bit what ffjord_forward gives for its batch alone.  Untaped.
function ffjord_forward_groups(h::FfjordHandle, x::ROCMatrix{Float32}, p::ROCVector{Float32}, e::Union{Nothing,ROCMatrix{Float32}},
                               Bs::Vector{Int32}, tspan; acc::Union{Nothing,ROCVector{Float64}} = nothing)
    n = length(Bs)
    logpx = similar(x, size(x, 2))
    nfe = Vector{Int64}(undef, n); status = Vector{Int32}(undef, n)
    GC.@preserve x p e logpx acc begin
        sum_ptr = acc === nothing ? C_NULL : devptr(acc)
        cnt_ptr = acc === nothing ? C_NULL : devptr(acc) + 8
        st = ccall((:rnde_ffjord_forward_groups, LIB), Cint,
                   (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ptr{Int32}, Float32, Float32, Int32, Ptr{Cvoid}, Ptr{Int64}, Ptr{Int32},
                    Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                   h.ptr, devptr(x), devptr(p), e === nothing ? C_NULL : devptr(e), n, Bs, Float32(tspan[1]), Float32(tspan[2]),
                   e === nothing ? 1 : 0, devptr(logpx), nfe, status, sum_ptr, cnt_ptr, _stream())
        st == 0 || error("rnde_ffjord_forward_groups status $st: ", _fferr(h.ptr))
    end
    return logpx, Int.(nfe), Int.(status)
end
# (dt, accepted) pairs of group g (0-based, as the library counts) of the last group call, flattened
function ffjord_group_steps(h::FfjordHandle, g::Integer)
    n = Ref{Int32}(0)
    ccall((:rnde_ffjord_group_steps, LIB), Cint, (Ptr{Cvoid}, Int32, Ptr{Float32}, Int32, Ref{Int32}), h.ptr, Int32(g), C_NULL, 0, n)
    steps = Vector{Float32}(undef, 2 * n[])
    st = ccall((:rnde_ffjord_group_steps, LIB), Cint, (Ptr{Cvoid}, Int32, Ptr{Float32}, Int32, Ref{Int32}), h.ptr, Int32(g), steps, n[], n)
    st == 0 || error("rnde_ffjord_group_steps status $st: ", _fferr(h.ptr))
    return steps
end

end # module
