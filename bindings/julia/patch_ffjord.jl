# patch_ffjord.jl -- the two call methods of TrackedFFJORD the FFJORD experiments use (reference src/models/ffjord.jl:68-135) and `sample`
# (:160-167), with their `solve` replaced by librnde.so.  SOURCE ONLY (no Julia in the build image).  Usage: include RNDE.jl, then this
# file, after `using RegNeuralDE` (see patch_neural_ode.jl).  Served: `dynamics = forw_n_back` of the ConcatSquash MLPDynamics of
# experiments/ffjord_gaussian.jl:48-107 with in_dims + 1 <= 64 and hsize <= 64, Tsit5; with RNDE_FFJORD_ENGINE[] = :tiled, in_dims <= 64 and
# hsize <= 112 (experiments/ffjord_tabular.jl's 43 -> 100).  Also served: the default forw_n_back (dynamics = nothing: Tracker.forward, then
# back) when the model is a chain of Flux.Dense layers -- a TDChain with time_dep = true or a Chain with time_dep = false, up to 8 layers, no
# width above 64, the six activations of RNDE.act_code -- through rnde_ffjord_create_chain (one engine, whatever RNDE_FFJORD_ENGINE[] says).
# Refused with an error that names the limit: any other model under the default forw_n_back, and widths above the engine's limit.  The {false} method's `regularize = true` (kinetic energy and Jacobian norm rows,
# ffjord.jl:53-66) runs the library's kinetic entries: in_dims + 3 <= 64 on the one-workgroup engine, the tiled engine's limits unchanged.
# `exact = true` (an extension: the reference has no forward exact call) solves with the exact trace -tr J instead of the Hutchinson estimate:
# no probe, the tiled engine or a chain model only, not together with `regularize = true` on a {false} layer.
# Both call methods are one Tracker node (RNDE.ffjord_solve): Tracker.gradient through the patched layer runs RNDE.ffjord_backward.
using Tracker, Flux, AMDGPU
using RegNeuralDE: TrackedFFJORD, TDChain, _convert_tspan

const RNDE_FFJORD_HANDLES = IdDict{Any,Dict{Int,RNDE.FfjordHandle}}()
# which engine new handles use: :workgroup (default) or :tiled (the tabular experiment's MLPDynamics(43, 100)); set before the first call
const RNDE_FFJORD_ENGINE = Ref(:workgroup)

# MLPDynamics(in, h) recognised by its three ConcatSquashLinear fields (layer_W of the first and second layer give in and h)
function _ffjord_dims(n::TrackedFFJORD)
    m = n.model
    hasproperty(m, :csl1) && hasproperty(m.csl1, :layer_W) ||
        error("RNDE: only the ConcatSquash MLPDynamics of experiments/ffjord_gaussian.jl (dynamics = forw_n_back) is served; the default forw_n_back (Tracker.forward) is not")
    h, d = size(m.csl1.layer_W)
    if RNDE_FFJORD_ENGINE[] === :tiled
        (d <= 64 && h <= 112) || error("RNDE: widths above the tiled engine's LDS limit are not served (in_dims <= 64, hidden <= 112); got ", (d, h))
    else
        (d + 1 <= 64 && h <= 64) || error("RNDE: widths above the chain engine's limit of 64 are not served (in_dims + 1 <= 64, hidden <= 64; ",
                                          "RNDE_FFJORD_ENGINE[] = :tiled serves wider models); got ", (d, h))
    end
    return d, h
end

# a Dense chain under the default dynamics: (dims, acts, time dependent), or nothing for any other model
_ffjord_is_chain(n::TrackedFFJORD) = (n.model isa TDChain || n.model isa Flux.Chain) && !hasproperty(n.model, :csl1)
function _ffjord_chain_layout(n::TrackedFFJORD)
    layers = collect(n.model.layers)
    td = n.model isa TDChain
    all(l -> l isa Flux.Dense, layers) ||
        error("RNDE: under the default forw_n_back (Tracker.forward) the model must be a chain of Flux.Dense layers (no leading element-wise map); got ",
              [typeof(l) for l in layers if !(l isa Flux.Dense)])
    td == n.time_dep || error("RNDE: time_dep = ", n.time_dep, " with a ", td ? "TDChain" : "Chain", ": Tracker.forward would call the model with the wrong number of arguments")
    dims = Int[size(layers[1].W, 2) - (td ? 1 : 0)]
    acts = Int[]
    for l in layers
        push!(dims, size(l.W, 1)); push!(acts, RNDE.act_code(l.σ))
    end
    (length(acts) <= 8 && maximum(dims) <= 64 && dims[1] + 1 <= 64 && dims[1] == dims[end]) ||
        error("RNDE: chain dynamics: up to 8 Dense layers, no width above the limit of 64, dims[1] + 1 <= 64 and dims[1] == dims[end]; got ", dims)
    return dims, acts, td
end

function _ffjord_handle(n::TrackedFFJORD{R}, B::Int) where {R}
    hs = get!(RNDE_FFJORD_HANDLES, n, Dict{Int,RNDE.FfjordHandle}())
    if _ffjord_is_chain(n)
        return get!(hs, B) do
            dims, acts, td = _ffjord_chain_layout(n)
            kw = n.kwargs
            RNDE.FfjordHandle(RNDE.ffjord_chain_config(dims, acts; time_dep = td ? 1 : 0, regularize = R ? 1 : 0, max_batch = B,
                                                       reltol = Float32(get(kw, :reltol, 1.4f-8)), abstol = Float32(get(kw, :abstol, 1.4f-8))))
        end
    end
    d, h = _ffjord_dims(n)
    get!(hs, B) do
        kw = n.kwargs
        RNDE.FfjordHandle(RNDE.FfjordConfig(d, h, 0, n.time_dep, R ? 1 : 0, 0, B, 0, Float32(get(kw, :reltol, 1.4f-8)), Float32(get(kw, :abstol, 1.4f-8)),
                                            1, 4096, 0); engine = RNDE_FFJORD_ENGINE[])
    end
end

function _ffjord_call(n::TrackedFFJORD{R}, x, p, e) where {R}
    H = _ffjord_handle(n, size(x, 2))
    logpx, sv = RNDE.ffjord_solve(H, x, p, e, _convert_tspan(n.tspan, p))
    z = zeros(Float32, 1, size(x, 2))
    return logpx, z, z, RNDE.FFJORD_NFE[H], (R ? (saveval = sv,) : nothing)      # (sv.saveval, as a SavedValues reads)
end

# regularize = true: logpx, lambda1 (kinetic energy), lambda2 (Jacobian norm) as 1 x B rows, all three on the Tracker tape
function _ffjord_call_kinetic(n::TrackedFFJORD{false}, x, p, e)
    chain = _ffjord_is_chain(n)
    d = chain ? _ffjord_chain_layout(n)[1][1] : _ffjord_dims(n)[1]
    chain && d + 3 > 64 && error("RNDE: chain dynamics with regularize = true: the state [z; l; lambda1; lambda2] must fit the limit of 64 rows; got in_dims = ", d)
    (chain || RNDE_FFJORD_ENGINE[] === :tiled || d + 3 <= 64) ||
        error("RNDE: TrackedFFJORD{false} with regularize = true (kinetic energy and Jacobian norm rows): the chain engine's limit of 64 rows holds ",
              "in_dims + 3 <= 64 (RNDE_FFJORD_ENGINE[] = :tiled serves in_dims <= 64); got in_dims = ", d)
    H = _ffjord_handle(n, size(x, 2))
    logpx, l1, l2 = RNDE.ffjord_solve_kinetic(H, x, p, e, _convert_tspan(n.tspan, p))
    return logpx, reshape(l1, 1, :), reshape(l2, 1, :), RNDE.FFJORD_NFE[H], nothing
end

# exact = true: logpx from the exact trace; the same 5-tuple, one Tracker node (RNDE.ffjord_solve_exact)
function _ffjord_call_exact(n::TrackedFFJORD{R}, x, p, kinetic::Bool) where {R}
    kinetic && error("RNDE: exact = true together with regularize = true on a {false} layer (kinetic energy and Jacobian norm rows) is not served: ",
                     "the Jacobian norm row is defined on the probe")
    (_ffjord_is_chain(n) || RNDE_FFJORD_ENGINE[] === :tiled) ||
        error("RNDE: exact = true is served on the tiled engine only (RNDE_FFJORD_ENGINE[] = :tiled)")
    H = _ffjord_handle(n, size(x, 2))
    logpx, sv = RNDE.ffjord_solve_exact(H, x, p, _convert_tspan(n.tspan, p))
    z = zeros(Float32, 1, size(x, 2))
    return logpx, z, z, RNDE.FFJORD_NFE[H], (R ? (saveval = sv,) : nothing)
end

# (e = nothing by default so that exact = true with a probe can be told apart and refused; the probe is drawn when the call needs one)
function (n::TrackedFFJORD{false})(x, p = n.p, e = nothing; regularize = false, exact = false)
    if exact
        e === nothing || error("RNDE: exact = true evaluates -tr J and takes no probe; call it without e")
        return _ffjord_call_exact(n, x, p, regularize)
    end
    e = e === nothing ? RNDE_randn(size(x)...) : e
    return regularize ? _ffjord_call_kinetic(n, x, p, e) : _ffjord_call(n, x, p, e)
end
function (n::TrackedFFJORD{true})(x, p = n.p, e = nothing; regularize = false, exact = false)
    if exact
        e === nothing || error("RNDE: exact = true evaluates -tr J and takes no probe; call it without e")
        return _ffjord_call_exact(n, x, p, false)
    end
    return _ffjord_call(n, x, p, e === nothing ? RNDE_randn(size(x)...) : e)
end

function RegNeuralDE.sample(n::TrackedFFJORD, indims::Int, p = n.p; nsamples::Int = 1)
    H = _ffjord_handle(n, nsamples)
    return RNDE.ffjord_sample(H, Tracker.data(p), RNDE_randn(indims, nsamples), _convert_tspan(n.tspan, p))
end

RNDE_randn(dims...) = AMDGPU.randn(Float32, dims...)

# The training step in one call.  The two lines of the experiments' loop (experiments/ffjord_tabular.jl:225-229, ffjord_gaussian.jl:224-225)
#
#     gs = Tracker.gradient(p -> loss_function(x, ffjord, p; λᵣ = λᵣ, notrack = false), ps...)
#     update_parameters!(ps, gs, opt)                    # opt = Optimiser(WeightDecay(1e-5), ADAM(1e-2))
#
# become, with m = zero(p), v = zero(p) made once and t = 1, 2, ... counted by the loop:
#
#     H = _ffjord_handle(ffjord, size(x, 2))
#     pbar, _, terms, reg, nfe = RNDE.ffjord_nll_grad(H, x, Tracker.data(ffjord.p), nothing, _convert_tspan(ffjord.tspan, ffjord.p);
#                                                     lambda_r = REGULARIZE ? λᵣ : 0f0, seed = t)     # terms[1] = -mean(logpx), on the device
#     RNDE.adam_wd_step!(Tracker.data(ffjord.p), pbar, m, v, t; eta = 1f-2, wd = 1f-5)
#
# (the {false} method with regularize = true: mode = 2, lambda_k and lambda_j the weights of mean(r1) and mean(r2); exact = true: mode = 1.)
# The logger's three numbers are Array(terms)[1] + reg, Array(terms)[1] and reg, read when they are wanted.
